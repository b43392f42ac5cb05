// bhray_accum_denoise.h — denoised stills (bhray_accum_read_denoised): an edge-avoiding a-trous filter over the accumulation's colour mean, guided by
// the means of its still passes.  What the engine (bhray_api.hip) passes to the kernels of bhray_accum_denoise.hip, and the functions - denoise_texel, denoise_pixel -
// that run include/bhray.h's rule on the device and on the host (bhray_accum_denoise_host).
#pragma once
#include "bhray_accum_passes.h"

namespace bhray {

// The filter's working images are planes of float4, one texel per pixel:
//   ct   (r, g, b, t): the colour C_i and its compressed luminance t_i; t == DENOISE_INVALID (-1.0f: a valid t is in [0, 1], -0 or a NaN) marks a pixel that is not
//        valid - it keeps r, g, b through every iteration; its alpha, which the plane does not hold, is C_0's
//   g0   (coverage mean xyz, closest approach mean); g1: position mean xyz; g2: escape mean xyz - the guides, never filtered; read and written only where the
//        guide set needs them
constexpr uint32_t DENOISE_INVALID_BITS = 0xbf800000u;            // -1.0f
constexpr uint32_t DENOISE_NEEDS_G0 = BHRAY_PASS_COVERAGE | BHRAY_PASS_GEOMETRY, DENOISE_NEEDS_G1 = BHRAY_PASS_POSITION, DENOISE_NEEDS_G2 = BHRAY_PASS_ESCAPE;

// the rule's constants: the guide set (never 0) and each sigma squared, formed once on the host
struct DenoiseRule { uint32_t guides; float s2_colour, s2_coverage, s2_closest, s2_position, s2_escape; };

BH_HD bool denoise_nonfinite(float x) { return (f2u(x) & 0x7f800000u) == 0x7f800000u; }
BH_HD bool denoise_valid_t(float t) { return f2u(t) != DENOISE_INVALID_BITS; }

// the adaptive stills' compressed luminance (accum_adapt_add_kernel's operations, include/bhray.h)
BH_HD float denoise_luminance(float r, float g, float b) {
    float Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    Y = Y < 0.0f ? 0.0f : Y;
    return Y >= 0x1p100f ? 1.0f : Y / (1.0f + Y);
}

// (r, g, b, t) of a colour whose alpha is `alpha`: valid iff alpha == 1 and r, g, b are finite
BH_HD float4 denoise_texel(float r, float g, float b, float alpha) {
    const bool valid = alpha == 1.0f && !denoise_nonfinite(r) && !denoise_nonfinite(g) && !denoise_nonfinite(b);
    return make_float4(r, g, b, valid ? denoise_luminance(r, g, b) : u2f(DENOISE_INVALID_BITS));
}

// the stop function E
BH_HD float denoise_stop(float d2, float s2) {
    const float q = d2 / s2;
    const float u = 1.0f - q;
    return u > 0.0f ? u * u : 0.0f;                               // false for a NaN
}

BH_HD float denoise_dist2(const float4& a, const float4& b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// One iteration's value of one pixel, include/bhray.h's rule word by word: the new (r, g, b, t) texel.  F answers the working images around the pixel:
// f.ct(a, b), f.g0(a, b), f.g1(a, b), f.g2(a, b) are the texels `a` taps right of and `b` taps below it (a, b in -2 .. 2; tap spacing is F's business); ct of a tap
// outside the frame carries the invalid mark, and a guide plane is asked only where the set needs it.
template <class F> BH_HD float4 denoise_pixel(const DenoiseRule& P, const F& f) {
    const float4 pc = f.ct(0, 0);
    if (!denoise_valid_t(pc.w)) return pc;
    const bool need0 = (P.guides & DENOISE_NEEDS_G0) != 0, need1 = (P.guides & DENOISE_NEEDS_G1) != 0, need2 = (P.guides & DENOISE_NEEDS_G2) != 0;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 p0 = need0 ? f.g0(0, 0) : zero, p1 = need1 ? f.g1(0, 0) : zero, p2 = need2 ? f.g2(0, 0) : zero;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f;
#pragma unroll
    for (int b = -2; b <= 2; b++) {
#pragma unroll
        for (int a = -2; a <= 2; a++) {
            const float4 qc = f.ct(a, b);
            if (!denoise_valid_t(qc.w)) continue;
            const float ha = a == 0 ? 0.375f : (a == 1 || a == -1) ? 0.25f : 0.0625f;
            const float hb = b == 0 ? 0.375f : (b == 1 || b == -1) ? 0.25f : 0.0625f;
            float w = ha * hb;
            const float dt = pc.w - qc.w;
            w = w * denoise_stop(dt * dt, P.s2_colour);
            if (need0) {
                const float4 q0 = f.g0(a, b);
                if (P.guides & BHRAY_PASS_COVERAGE) w = w * denoise_stop(denoise_dist2(p0, q0), P.s2_coverage);
                if (P.guides & BHRAY_PASS_GEOMETRY) { const float d = p0.w - q0.w; w = w * denoise_stop(d * d, P.s2_closest); }
            }
            if (need1) w = w * denoise_stop(denoise_dist2(p1, f.g1(a, b)), P.s2_position);
            if (need2) w = w * denoise_stop(denoise_dist2(p2, f.g2(a, b)), P.s2_escape);
            ax = ax + w * qc.x; ay = ay + w * qc.y; az = az + w * qc.z;
            ws = ws + w;
        }
    }
    if (!(ws > 0.0f)) return pc;
    return denoise_texel(ax / ws, ay / ws, az / ws, 1.0f);
}

// the working images of a ctx's denoiser, frame_w * frame_h texels each; g[i] is nullptr where the guide set does not need it
struct DenoisePlanes { float4* ct[2]; float4* g[3]; };

// nullptr: p is acceptable with the pass set `set` (never 0); else why not
const char* still_denoise_error(const bhray_still_denoise* p, uint32_t set);
// the rule's constants for an accepted p (nullptr: the defaults) under the pass set `set`
void denoise_rule_fill(DenoiseRule& r, const bhray_still_denoise* p, uint32_t set);

// mean[p] = the colour mean of sum[p] by accum_mean_kernel's operations; ct[p] = its (r, g, b, t); g0 / g1 / g2[p] = the guide means of the planes the set needs.
// Planes that the set does not need are neither read nor written.  Enqueues only.
hipError_t launch_denoise_prepare(const float4* sum, const AccumPassPlanes& planes, uint32_t guides, float4* mean, float4* ct, float4* g0, float4* g1, float4* g2,
                                  uint32_t npix, hipStream_t s);
// One a-trous iteration at tap spacing `step` (1, 2, 4, 8 or 16): dst = the iteration's (r, g, b, t) image of src.  last: dst takes (r, g, b, alpha) instead - alpha 1
// for a pixel that was valid in src, mean[p].w otherwise - and out16 (may be nullptr) the same rounded to RGBA16F by accum_mean_kernel's conversion.  Enqueues only.
hipError_t launch_denoise_atrous(const DenoiseRule& rule, const float4* src, const float4* g0, const float4* g1, const float4* g2, const float4* mean, float4* dst,
                                 uint2* out16, uint32_t frame_w, uint32_t frame_h, uint32_t step, bool last, hipStream_t s);

}  // namespace bhray
