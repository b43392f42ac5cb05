// bhray_accum_stars.hip — the kernel of point stars in stills (bhray_accum_set_stars) and the host form of its neighbour rule.
//
//   accum_star_kernel   between a launch's trace and its add (accum_add_kernel or accum_filter_add_kernel): every sample image of the launch becomes its starred
//                       image T - a pixel that accepted a star under §23's rules is (min(resolve(pixel) + acc * gain, 65504), 1), every other pixel keeps its bits
//
// star_kernel's shape: a block is four waves on a 64 x 4 pixel tile of ONE sample (blockIdx.z); the 66 x 6 result texels around it go into LDS (6336 bytes), the
// 65 x 5 corners of the tile's pixels are formed once per block into LDS (5200 bytes), validity in .w, then star_pixel of bhray_stars.h per lane.  The halo load takes
// x modulo W under wrap_x (a 360 degree equirect still is periodic in x); otherwise, and always in y, a texel outside the frame is (0, 0, 0, 1): not a direction pixel.
// Samples are independent - the kernel writes T, not the sum -, so the grid's z is the sample and a small frame's launch still fills the device.  Every in-frame pixel
// of T is written; the sky texture is read only by pixels that accepted a star.  Every loop is bounded as star_kernel's, every index inside its allocation whatever the
// results hold: the halo's coordinates are tested against the frame after the wrap, the cell coordinates are clamped before they index the prefix array.
// Translation unit of its own, so that no pre-existing kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bhray_accum_stars.h"
#include "bhray_tex.h"

namespace bhray {
namespace {

constexpr int TILE_W = 64, TILE_H = 4, TILE_P = TILE_W + 2, CORN_P = TILE_W + 1;
constexpr unsigned GRID_Z_MAX = 65535u;

__global__ __launch_bounds__(256) void accum_star_kernel(const StarSet S, const TexDev sky, const float4* __restrict__ results, float4* __restrict__ T, int W, int H, int wrap_x) {
    __shared__ float4 tile[(TILE_H + 2) * TILE_P];
    __shared__ float4 corn[(TILE_H + 1) * CORN_P];
    const size_t base = (size_t)blockIdx.z * ((size_t)W * (size_t)H);
    const float4* __restrict__ src = results + base;
    const int bx = (int)blockIdx.x * TILE_W, by = (int)blockIdx.y * TILE_H;
    for (int i = (int)threadIdx.x; i < (TILE_H + 2) * TILE_P; i += 256) {
        const int ly = i / TILE_P, lx = i - ly * TILE_P;
        int gx = bx + lx - 1;
        const int gy = by + ly - 1;
        if (wrap_x) { if (gx < 0) gx += W; else if (gx >= W) gx -= W; }   // columns -1 and W are columns W - 1 and 0 of the same sample
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 1.0f);                  // outside the frame: not a direction pixel
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = src[(size_t)gy * (size_t)W + (size_t)gx];
        tile[i] = v;
    }
    __syncthreads();
    // corner (lx, ly) of the tile: the upper left corner of tile pixel (lx, ly), between tile texels (lx, ly), (lx + 1, ly), (lx, ly + 1), (lx + 1, ly + 1) (halo offset 1)
    for (int i = (int)threadIdx.x; i < (TILE_H + 1) * CORN_P; i += 256) {
        const int ly = i / CORN_P, lx = i - ly * CORN_P;
        const int t = ly * TILE_P + lx;
        F3 c;
        const bool ok = star_corner(tile[t], tile[t + 1], tile[t + TILE_P], tile[t + TILE_P + 1], c);
        corn[i] = make_float4(c.x, c.y, c.z, ok ? 1.0f : 0.0f);
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (TILE_W - 1), ty = (int)threadIdx.x >> 6;
    const int gx = bx + tx, gy = by + ty;
    if (gx >= W || gy >= H) return;
    const int ci = ty * CORN_P + tx;
    const float4 k00 = corn[ci], k10 = corn[ci + 1], k01 = corn[ci + CORN_P], k11 = corn[ci + CORN_P + 1];
    float4 p = tile[(ty + 1) * TILE_P + tx + 1];                         // the pixel's own result: what T keeps unless a star arrives
    if (k00.w != 0.0f && k10.w != 0.0f && k01.w != 0.0f && k11.w != 0.0f) {
        F3 acc;
        const uint32_t n = star_pixel(S, f3(p.x, p.y, p.z), f3(k00.x, k00.y, k00.z), f3(k10.x, k10.y, k10.z), f3(k01.x, k01.y, k01.z), f3(k11.x, k11.y, k11.z), acc, nullptr);
        if (n != 0) {
            const float4 b = resolve(sky, p);                            // a direction pixel (rule 1): the accumulation's binary32 sky^4, alpha 1
            p = make_float4(min_(b.x + acc.x * S.gain, 65504.0f), min_(b.y + acc.y * S.gain, 65504.0f), min_(b.z + acc.z * S.gain, 65504.0f), 1.0f);
        }
    }
    T[base + (size_t)gy * (size_t)W + (size_t)gx] = p;
}

}  // namespace

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_accum_stars(const StarSet& S, const TexDev& sky, const float4* results, float4* T, uint32_t frame_w, uint32_t frame_h, uint32_t k, int wrap_x, hipStream_t s) {
    if (frame_w == 0 || frame_h == 0 || k == 0) return hipSuccess;
    const unsigned gx = (frame_w + TILE_W - 1) / TILE_W, gy = (frame_h + TILE_H - 1) / TILE_H;
    if (gy > 65535u || frame_w > 32767u || !S.stars || !S.prefix || S.G < 1 || S.G > 1024 || (S.G & (S.G - 1)) != 0 || !results || !T || !sky.rgba || sky.w < 1 || sky.h < 1)
        return hipErrorInvalidValue;
    const size_t npix = (size_t)frame_w * frame_h;
    for (uint32_t j0 = 0; j0 < k;) {                                     // a grid's z holds 65535 samples; the samples are independent, so more of them take more launches
        const uint32_t kz = std::min(k - j0, GRID_Z_MAX);
        (void)hipGetLastError();
        hipLaunchKernelGGL(accum_star_kernel, dim3(gx, gy, kz), dim3(256), 0, s, S, sky, results + (size_t)j0 * npix, T + (size_t)j0 * npix, (int)frame_w, (int)frame_h, wrap_x ? 1 : 0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        j0 += kz;
    }
    return hipSuccess;
}

}  // namespace bhray

// bhray_stars_resolve_host with the wrap of §24: one change to how a neighbour outside [0, w) is fetched
extern "C" int bhray_accum_stars_resolve_host(const float* results, uint32_t w, uint32_t h, int32_t wrap_x, const bhray_star* stars, uint32_t n, const bhray_star_params* params,
                                              float* add) {
    if (!add) return BHRAY_E_INVALID;
    return bhray::stars_resolve_host(results, w, h, wrap_x != 0, stars, n, params, add, nullptr);
}
