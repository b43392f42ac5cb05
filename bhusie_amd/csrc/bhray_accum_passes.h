// bhray_accum_passes.h — still passes (bhray_accum_set_passes): per-pixel coverage, geometry, position and escape maps summed beside the accumulation
// image.  What the engine (bhray_api.hip) passes to the kernels of bhray_accum_passes.hip, and the one function - accum_pass_value - that forms a sample's
// contribution on the device and on the host (bhray_accum_pass_values).
#pragma once
#include "bhray_accum.h"

namespace bhray {

constexpr uint32_t ACCUM_PASS_COUNT = 4;                          // the bits of BHRAY_PASS_ALL; plane i belongs to bit 1u << i

// A sample's contribution to `pass` (exactly one BHRAY_PASS_* bit), include/bhray.h's rule word by word.  R: the trace's result; qa, qb: the two 16-byte halves of
// its record as they lie in memory - (position, hit) and (triangle, iterations, closest, transmittance), the integers as their bit patterns -; d: the direction half
// of the ray as it was traced (read for BHRAY_PASS_ESCAPE only).  false: the sample is skipped (R.x, R.y or R.z not finite) and v is untouched.
BH_HD bool accum_pass_value(uint32_t pass, const float4& R, const float4& qa, const float4& qb, const float4& d, float4& v) {
    if ((f2u(R.x) & 0x7f800000u) == 0x7f800000u || (f2u(R.y) & 0x7f800000u) == 0x7f800000u || (f2u(R.z) & 0x7f800000u) == 0x7f800000u) return false;
    const uint32_t kind = f2u(qa.w) & 0xffu;
    v = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (kind == BHRAY_HIT_UNUSABLE) return true;                  // a finite black sample with a zero vector in every pass
    if (pass == BHRAY_PASS_COVERAGE) {
        v.x = kind == BHRAY_HIT_HORIZON ? 1.0f : 0.0f; v.y = kind == BHRAY_HIT_DISK ? 1.0f : 0.0f; v.z = kind == BHRAY_HIT_MESH ? 1.0f : 0.0f;
    }
    else if (pass == BHRAY_PASS_GEOMETRY) { v.x = qb.z; v.y = (float)f2u(qb.y); v.z = qb.w; }
    else if (pass == BHRAY_PASS_POSITION) {
        if (kind == BHRAY_HIT_DISK || kind == BHRAY_HIT_MESH) { v.x = qa.x; v.y = qa.y; v.z = qa.z; }
    }
    else {                                                        // BHRAY_PASS_ESCAPE
        if (R.w == 0.0f) { v.x = R.x; v.y = R.y; v.z = R.z; }     // entered the sphere, left it, hit nothing: the final direction
        else if (kind == BHRAY_HIT_NONE) { v.x = d.x; v.y = d.y; v.z = d.z; }   // the loop ended at i <= 5 and the shader resolved the sky itself: the generated direction
    }
    return true;
}

// the sum planes of an accumulation: plane[i] for bit 1u << i, nullptr where the bit is not in the set
struct AccumPassPlanes { float4* plane[ACCUM_PASS_COUNT]; };

// The box form: for every pixel p and every pass of `passes`, plane[p] += (v, 1) over the launch's samples j = 0 .. k - 1 in that order - results j * npix + p, the
// record and the ray behind it (two float4 each).  rays may be nullptr unless BHRAY_PASS_ESCAPE is in the set.  Enqueues only.
hipError_t launch_accum_passes_add(const float4* results, const float4* records, const float4* rays, const AccumPassPlanes& planes, uint32_t passes, uint32_t npix,
                                   uint32_t k, hipStream_t s);
// The filtered form's first half: images[i] = (v, 1) of `pass` for ray i = 0 .. n - 1, all-NaN for a skipped sample - what launch_accum_filter_add then sums into
// that pass's plane (alpha 1: its resolve never fires; NaN: its own skip).  Enqueues only.
hipError_t launch_accum_passes_form(const float4* results, const float4* records, const float4* rays, uint32_t pass, float4* images, size_t n, hipStream_t s);

}  // namespace bhray
