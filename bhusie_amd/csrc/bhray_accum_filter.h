// bhray_accum_filter.h — still pixel filters (bhray_accum_set_filter): the accumulation image's reconstruction filter.  What the engine (bhray_api.hip)
// passes to the kernel of bhray_accum_filter.hip, and the one function - accum_filter_tap - that forms a sample's ten weights on the device and on the host.
#pragma once
#include "bhray_accum.h"

namespace bhray {

// bhray_still_filter as the kernel reads it: every member formed on the host (accum_filter_fill), the cubic's coefficients in binary64 and rounded once
struct AccumFilter {
    uint32_t kind;             // BHRAY_FILTER_TENT or BHRAY_FILTER_CUBIC (BHRAY_FILTER_BOX: tap 2 weighs 1)
    float radius;              // TENT
    float inv;                 // CUBIC: 2.0f / radius
    float p3, p2, p0;          // CUBIC, x < 1
    float q3, q2, q1, q0;      // CUBIC, 1 <= x < 2
};

// k(t), t = |tap position| >= 0: include/bhray.h's contract, operation by operation (the TU is compiled -ffp-contract=off)
BH_HD float accum_filter_k(const AccumFilter& f, float t) {
    if (f.kind == BHRAY_FILTER_TENT) {
        const float a = t / f.radius;
        return a < 1.0f ? 1.0f - a : 0.0f;
    }
    const float x = t * f.inv;
    if (x < 1.0f) return ((f.p3 * x + f.p2) * (x * x)) + f.p0;
    if (x < 2.0f) return (((f.q3 * x + f.q2) * x + f.q1) * x) + f.q0;
    return 0.0f;
}

// Weight n of sample s, n = 0 .. 9: wx[n] for n < 5, wy[n - 5] otherwise - tap i = n % 5 - 2 at float(i) + dx (dy)
BH_HD float accum_filter_tap(const AccumFilter& f, uint32_t s, uint32_t n) {
    float dx, dy;
    accum_offset(s, dx, dy);
    const uint32_t m = n < 5u ? n : n - 5u;
    if (f.kind == BHRAY_FILTER_BOX) return m == 2u ? 1.0f : 0.0f;
    const float t = (float)((int)m - 2) + (n < 5u ? dx : dy);
    return accum_filter_k(f, fabsf(t));
}

// nullptr, or why bhray_accum_set_filter refuses the struct (include/bhray.h)
const char* still_filter_error(const bhray_still_filter* filter);
// the kernel's constants of a struct that still_filter_error passes
void accum_filter_fill(AccumFilter& f, const bhray_still_filter& filter);
// The filtered form of launch_accum_add: for j = 0 .. k - 1 in that order, sum[p] += c, c the 5 x 5 stencil (weights of sample s0 + j) over V - the resolved result
// j * npix + p' of the pixels p' around p, zeros outside the frame and where the colour is not finite; sum[p].w collects the weight.  f.kind is not the box.
// Enqueues only.
hipError_t launch_accum_filter_add(const TexDev& sky, const AccumFilter& f, const float4* results, float4* sum, uint32_t frame_w, uint32_t frame_h, uint32_t s0, uint32_t k,
                                   hipStream_t s);

}  // namespace bhray
