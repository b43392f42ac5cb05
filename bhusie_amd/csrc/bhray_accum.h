// bhray_accum.h — the accumulation image (bhray_accum_*): what the engine (bhray_api.hip) passes to the kernels of bhray_accum.hip.
#pragma once
#include "bhray_internal.h"
#include "bhray_math.h"

namespace bhray {

// Sample s's sub-pixel offset, the same for every pixel: the R2 sequence in integer arithmetic - the 32-bit fractions of s / rho and s / rho^2 (rho the
// plastic number), started at one half - cut to 24 bits, so that the conversion, the scaling and the subtraction are exact in binary32 and host and device
// agree to the bit.  Sample 0: (0, 0), the pixel centre; every offset lies in [-0.5, 0.5).
BH_HD void accum_offset(uint32_t s, float& dx, float& dy) {
    const uint32_t u = 0x80000000u + s * 0xC13FA9A9u, v = 0x80000000u + s * 0x91E10DA5u;
    dx = (float)(u >> 8) * 0x1p-24f - 0.5f;
    dy = (float)(v >> 8) * 0x1p-24f - 0.5f;
}

// create_ray (ray.wgsl:269-285) on the ladder's last level for the pixels of the frame: the camera members of a frame's FrameParams (derive_frame) and the level's
// constants, formed on the host with the frames' operations
struct AccumGen {
    float cam[3], right[3], up[3], fwd_ff[3];
    float half_w, half_h;      // float(lw - 1) * 0.5f, float(lh - 1) * 0.5f
    float increment;           // 1.0f / float(min(lw - 1, lh - 1))
    uint32_t crop_x, crop_y, frame_w;
    uint32_t npix;             // frame_w * frame_h
    uint32_t s0, k;            // samples s0 .. s0 + k - 1
};
// records (s - s0) * npix + p of `rays` (two float4 each): the ray of sample s through frame pixel p.  k * npix <= 2^26.  Enqueues only.
hipError_t launch_accum_gen(const AccumGen& g, float4* rays, hipStream_t s);
// sum[p] += resolve(results[j * npix + p]) for j = 0 .. k - 1 in that order: alpha == 0 becomes sky^4 (the sky pass's operations, kept in binary32), a sample whose
// colour is not finite is skipped, sum[p].w counts the samples taken.  Enqueues only.
hipError_t launch_accum_add(const TexDev& sky, const float4* results, float4* sum, uint32_t npix, uint32_t k, hipStream_t s);
// mean[p] = (sum.xyz / sum.w, 1), or zeros where sum.w == 0; mean16 (may be nullptr): the same rounded to RGBA16F, nearest even.  Enqueues only.
hipError_t launch_accum_mean(const float4* sum, float4* mean, uint2* mean16, uint32_t npix, hipStream_t s);

}  // namespace bhray
