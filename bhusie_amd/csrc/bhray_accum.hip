// bhray_accum.hip — the kernels of the accumulation image (bhray_accum_*): supersampled stills.
//
//   accum_gen_kernel    the bhray_ray records of K consecutive samples of every frame pixel, sample-major (what the ray-list trace kernels read)
//   accum_add_kernel    resolve (alpha == 0 -> sky^4, binary32) and add the K results of a pixel to its sum, in sample order
//   accum_mean_kernel   sum -> mean, RGBA32F and RGBA16F (the display pass's input)
//
// One thread per pixel (per record in the generator), consecutive lanes on consecutive pixels, every access one float4: the kernels move 32 / 48 / 40 bytes per
// pixel and do little else, so they are HBM-bound by construction.  No atomics: a pixel's sum has one writer, and the order of its additions is the sample order
// whatever the grouping of samples into launches.  Translation unit of its own, so that no pre-existing kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "bhray_accum.h"
#include "bhray_tex.h"

namespace bhray {
namespace {

// record i = j * npix + p: sample s0 + j through frame pixel p = y * frame_w + x, i.e. pixel (crop_x + x, crop_y + y) of the last level
__global__ __launch_bounds__(256) void accum_gen_kernel(const AccumGen g, float4* __restrict__ rays) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.k * g.npix) return;
    const uint32_t j = (uint32_t)(i / g.npix), p = (uint32_t)(i - (size_t)j * g.npix);
    const uint32_t y = p / g.frame_w, x = p - y * g.frame_w;
    float dx, dy;
    accum_offset(g.s0 + j, dx, dy);
    const float px = (float)(g.crop_x + x) + dx, py = (float)(g.crop_y + y) + dy;
    // create_ray, ray.wgsl:269-285, as the trace kernels' refill forms it (right / up / fwd_ff and the level's constants from the host)
    const float posx = (2.0f * (px - g.half_w)) * g.increment;
    const float posy = (2.0f * (py - g.half_h)) * g.increment;
    const F3 rdir = normalize((ld3(g.right) * posx + ld3(g.up) * posy) + ld3(g.fwd_ff));
    rays[2 * i] = make_float4(g.cam[0], g.cam[1], g.cam[2], 0.0f);
    rays[2 * i + 1] = make_float4(rdir.x, rdir.y, rdir.z, 0.0f);
}

__global__ __launch_bounds__(256) void accum_add_kernel(const TexDev sky, const float4* __restrict__ results, float4* __restrict__ sum, uint32_t npix, uint32_t k) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    float4 acc = sum[p];
    for (uint32_t j = 0; j < k; j++) {
        const float4 r = resolve(sky, results[(size_t)j * npix + p]);
        if (finite_(r.x) && finite_(r.y) && finite_(r.z)) { acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += 1.0f; }
    }
    sum[p] = acc;
}

__global__ __launch_bounds__(256) void accum_mean_kernel(const float4* __restrict__ sum, float4* __restrict__ mean, uint2* __restrict__ mean16, uint32_t npix) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 a = sum[p];
    const float4 m = a.w == 0.0f ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(a.x / a.w, a.y / a.w, a.z / a.w, 1.0f);
    mean[p] = m;
    if (mean16) {
        const uint32_t lo = (uint32_t)__half_as_ushort(__float2half_rn(m.x)) | ((uint32_t)__half_as_ushort(__float2half_rn(m.y)) << 16);
        const uint32_t hi = (uint32_t)__half_as_ushort(__float2half_rn(m.z)) | ((uint32_t)__half_as_ushort(__float2half_rn(m.w)) << 16);
        mean16[p] = make_uint2(lo, hi);
    }
}

}  // namespace

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_accum_gen(const AccumGen& g, float4* rays, hipStream_t s) {
    const size_t n = (size_t)g.k * g.npix;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.frame_w == 0) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_gen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, rays);
    return hipGetLastError();
}

hipError_t launch_accum_add(const TexDev& sky, const float4* results, float4* sum, uint32_t npix, uint32_t k, hipStream_t s) {
    if (npix == 0 || k == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_add_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, sky, results, sum, npix, k);
    return hipGetLastError();
}

hipError_t launch_accum_mean(const float4* sum, float4* mean, uint2* mean16, uint32_t npix, hipStream_t s) {
    if (npix == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_mean_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, sum, mean, mean16, npix);
    return hipGetLastError();
}

}  // namespace bhray

extern "C" void bhray_accum_sample_offset(uint32_t s, float* dx, float* dy) {
    float x, y;
    bhray::accum_offset(s, x, y);
    if (dx) *dx = x;
    if (dy) *dy = y;
}
