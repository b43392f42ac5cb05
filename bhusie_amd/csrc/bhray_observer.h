// bhray_observer.h — the moving observer of stills (bhray_accum_set_observer): Lorentz aberration of every generated look direction and the D^4 beam
// of every resolved sample.  What the engine (bhray_api.hip) passes to the kernels of bhray_observer.hip, and the one function - observer_record - that forms a sample's
// boosted record and its beam on the device and on the host.
#pragma once
#include "bhray_stillcam.h"

namespace bhray {

// the observer's constants, formed on the host once per call (observer_fill), one rounded binary32 operation each
struct ObserverDev {
    float b[3];                // beta: the velocity in the static frame, world axes, units of c
    float ig;                  // sqrtf(1 - bb), bb = (bx*bx + by*by) + bz*bz: 1 / gamma
    float k;                   // g / (g + 1), g = 1 / ig
};

// include/bhray.h's rule for one look direction n' of the observer's rest frame (not all zero): the static-frame direction n and the beam D^4, operation by operation
// (the TUs that call it are compiled -ffp-contract=off)
BH_HD void observer_boost(const ObserverDev& o, float& nx, float& ny, float& nz, float& beam) {
    const float c = (o.b[0] * nx + o.b[1] * ny) + o.b[2] * nz;
    const float a = o.k * c - 1.0f;
    const float q = 1.0f / (1.0f - c);
    const float vx = ((nx * o.ig) + (o.b[0] * a)) * q;
    const float vy = ((ny * o.ig) + (o.b[1] * a)) * q;
    const float vz = ((nz * o.ig) + (o.b[2] * a)) * q;
    const float r = 1.0f / sqrtf((vx * vx + vy * vy) + vz * vz);
    nx = vx * r; ny = vy * r; nz = vz * r;
    const float D = o.ig * q;                                     // nu_observed / nu_static = 1 / (gamma (1 - b.n'))
    const float D2 = D * D;
    beam = D2 * D2;
}

// The record of sample s through pixel (lx, ly) of the last level under the still camera of g, seen by the observer o: still_record's origin, its direction boosted,
// and the beam of the record.  An all-zero rest-frame direction (outside a fisheye's circle) passes unchanged with beam 1.
BH_HD void observer_record(const StillGen& g, const ObserverDev& o, uint32_t lx, uint32_t ly, uint32_t s, float4& origin, float4& direction, float& beam) {
    still_record(g, lx, ly, s, origin, direction);
    beam = 1.0f;
    if (direction.x == 0.0f && direction.y == 0.0f && direction.z == 0.0f) return;
    observer_boost(o, direction.x, direction.y, direction.z, beam);
}

// nullptr, or why bhray_accum_set_observer refuses the struct (include/bhray.h)
const char* observer_error(const bhray_observer* obs);
// whether the observer is at rest (an all-zero velocity, whatever `beaming` says): the accumulation then runs the generators it ran without one, and no beam stage
inline bool observer_at_rest(const bhray_observer& obs) { return obs.velocity[0] == 0.0f && obs.velocity[1] == 0.0f && obs.velocity[2] == 0.0f; }
// the constants of a moving observer
void observer_fill(ObserverDev& o, const bhray_observer& obs);
// launch_still_gen / launch_still_gen_list (bhray_stillcam.h) with every record through observer_record: the same layouts, the same limits.  Enqueue only.
hipError_t launch_observer_gen(const StillGen& g, const ObserverDev& o, float4* rays, hipStream_t s);
hipError_t launch_observer_gen_list(const StillGen& g, const ObserverDev& o, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state, float4* rays, hipStream_t s);
// The beam stage, in place on the launch's results (or its starred images), indexed as the generators' records: img[r] with w == 0 becomes the accumulation's resolve
// (binary32 sky^4, alpha 1), then x, y, z are multiplied by the record's beam - recomputed through observer_record, so the generator's bits - and w is kept.  A record
// whose rest-frame direction is all zero is not touched.  Enqueue only.
hipError_t launch_observer_beam(const StillGen& g, const ObserverDev& o, const TexDev& sky, float4* img, hipStream_t s);
hipError_t launch_observer_beam_list(const StillGen& g, const ObserverDev& o, const TexDev& sky, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state,
                                     float4* img, hipStream_t s);

}  // namespace bhray
