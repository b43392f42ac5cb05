// bhray_skyfilter.hip — the kernels of the footprint-filtered sky pass (bhray_set_sky_filter).
//
//   sky_pyramid_first_kernel   RGBA8 sky texture -> level 1: the box mean of (byte / 255)^4 over 2 x 2 texels, RGBA16F
//   sky_pyramid_next_kernel    level l -> level l + 1 from the stored halves
//   sky_filter_kernel          the sky pass with 1, 2, 4 or 8 taps per direction pixel along the longer of its two neighbour differences, each tap a blend of two levels
//
// sky_filter_kernel is a stencil over the RGBA32F frame plus gathers from the pyramid.  A block is four waves on a 64 x 4 pixel tile: a wave is 64 consecutive pixels
// of one row, so the frame is read with 16-byte loads (1 KiB per wave instruction) and the image written with 8-byte stores, as sky_kernel does.  The four
// neighbours come from an LDS tile of 66 x 6 float4 (6336 bytes: every block that fits a CU by registers fits by LDS) that the block fills once, halo included; the
// halo rows are the interior rows of the blocks above and below, which run at about the same time, so they are L2 hits and each frame pixel comes from HBM about
// once.  (Cross-lane moves would serve the horizontal pair only: the vertical pair lives in other waves.)  A pixel that is not filtered runs sky_kernel's operations
// on its own direction - one tap of level 0 - so its bits are sky_kernel's.  Translation unit of its own, so that no pre-existing kernel's registers or schedule
// can move with it.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "bhray_skyfilter.h"
#include "bhray_tex.h"

namespace bhray {
namespace {

constexpr int TILE_W = 64, TILE_H = 4, TILE_P = TILE_W + 2;      // tile of a block, and the pitch of its LDS copy with the one-pixel halo

__device__ __forceinline__ float h2f(uint32_t bits16) { return __half2float(__ushort_as_half((unsigned short)bits16)); }
__device__ __forceinline__ uint32_t f2h(float x) { return (uint32_t)__half_as_ushort(__float2half_rn(x)); }
__device__ __forceinline__ uint2 pack16(float x, float y, float z, float w) { return make_uint2(f2h(x) | (f2h(y) << 16), f2h(z) | (f2h(w) << 16)); }
__device__ __forceinline__ F3 texel16(const uint2* __restrict__ lv, int w, int x, int y) {
    const uint2 q = lv[(size_t)y * (size_t)w + (size_t)x];
    return f3(h2f(q.x & 0xffffu), h2f(q.x >> 16), h2f(q.y & 0xffffu));
}
__device__ __forceinline__ float pow4(float s) { return (s * s) * (s * s); }

// the box mean of four values as every level forms it
__device__ __forceinline__ float box(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

__global__ __launch_bounds__(256) void sky_pyramid_first_kernel(const TexDev sky, uint2* __restrict__ dst, int dw, int dh) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)dw * (size_t)dh) return;
    const int y = (int)(i / (size_t)dw), x = (int)(i - (size_t)y * (size_t)dw);
    const int x0 = 2 * x, y0 = 2 * y, x1 = x0 + 1 < sky.w ? x0 + 1 : sky.w - 1, y1 = y0 + 1 < sky.h ? y0 + 1 : sky.h - 1;
    const float4 a = texel<false>(sky, x0, y0), b = texel<false>(sky, x1, y0), c = texel<false>(sky, x0, y1), d = texel<false>(sky, x1, y1);
    dst[i] = pack16(box(pow4(a.x), pow4(b.x), pow4(c.x), pow4(d.x)), box(pow4(a.y), pow4(b.y), pow4(c.y), pow4(d.y)),
                    box(pow4(a.z), pow4(b.z), pow4(c.z), pow4(d.z)), 1.0f);
}

__global__ __launch_bounds__(256) void sky_pyramid_next_kernel(const uint2* __restrict__ src, int sw, int sh, uint2* __restrict__ dst, int dw, int dh) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)dw * (size_t)dh) return;
    const int y = (int)(i / (size_t)dw), x = (int)(i - (size_t)y * (size_t)dw);
    const int x0 = 2 * x, y0 = 2 * y, x1 = x0 + 1 < sw ? x0 + 1 : sw - 1, y1 = y0 + 1 < sh ? y0 + 1 : sh - 1;
    const F3 a = texel16(src, sw, x0, y0), b = texel16(src, sw, x1, y0), c = texel16(src, sw, x0, y1), d = texel16(src, sw, x1, y1);
    dst[i] = pack16(box(a.x, b.x, c.x, d.x), box(a.y, b.y, c.y, d.y), box(a.z, b.z, c.z, d.z), 1.0f);
}

// S_l(u, v): level 0 - sky_kernel's sample and power; level l >= 1 - the same unit_coord and mix_ over the level's halves, no power
__device__ __forceinline__ F3 sample_level(const TexDev& sky, const SkyPyr& pyr, int l, float u, float v) {
    if (l == 0) {
        const float4 sc = sample_bilinear<false>(sky, u, v);
        return f3(pow4(sc.x), pow4(sc.y), pow4(sc.z));
    }
    const int w = sky_pyr_dim(sky.w, l), h = sky_pyr_dim(sky.h, l);
    const uint2* __restrict__ lv = pyr.base + pyr.off[l];
    int x0, x1, y0, y1;
    const float fx = unit_coord(u, w, x0, x1);
    const float fy = unit_coord(v, h, y0, y1);
    const F3 a = texel16(lv, w, x0, y0), b = texel16(lv, w, x1, y0), c = texel16(lv, w, x0, y1), d = texel16(lv, w, x1, y1);
    return f3(mix_(mix_(a.x, b.x, fx), mix_(c.x, d.x, fx), fy), mix_(mix_(a.y, b.y, fx), mix_(c.y, d.y, fx), fy), mix_(mix_(a.z, b.z, fx), mix_(c.z, d.z, fx), fy));
}

__global__ __launch_bounds__(256) void sky_filter_kernel(const TexDev sky, const SkyPyr pyr, const float4* __restrict__ src, uint2* __restrict__ dst, int W, int H) {
    __shared__ float4 tile[(TILE_H + 2) * TILE_P];
    const int bx = (int)blockIdx.x * TILE_W, by = (int)blockIdx.y * TILE_H;
    for (int i = (int)threadIdx.x; i < (TILE_H + 2) * TILE_P; i += 256) {
        const int ly = i / TILE_P, lx = i - ly * TILE_P;
        const int gx = bx + lx - 1, gy = by + ly - 1;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 1.0f);                  // outside the frame: not a direction pixel
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = src[(size_t)gy * (size_t)W + (size_t)gx];
        tile[i] = v;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (TILE_W - 1), ty = (int)threadIdx.x >> 6;
    const int gx = bx + tx, gy = by + ty;
    if (gx >= W || gy >= H) return;
    const int ci = (ty + 1) * TILE_P + tx + 1;
    float4 p = tile[ci];
    if (p.w == 0.0f) {                                                   // sky.wgsl:19
        const F3 d = f3(p.x, p.y, p.z);
        // 1. one-sided neighbour differences: right before left, below before above, direction pixels only
        const float4 nr = tile[ci + 1], nl = tile[ci - 1], nd = tile[ci + TILE_P], nu = tile[ci - TILE_P];
        F3 dh = f3(0.0f, 0.0f, 0.0f), dv = f3(0.0f, 0.0f, 0.0f);
        if (nr.w == 0.0f) dh = f3(nr.x, nr.y, nr.z) - d; else if (nl.w == 0.0f) dh = f3(nl.x, nl.y, nl.z) - d;
        if (nd.w == 0.0f) dv = f3(nd.x, nd.y, nd.z) - d; else if (nu.w == 0.0f) dv = f3(nu.x, nu.y, nu.z) - d;
        // 2. footprints in equatorial texels
        const float PI_F = 3.1415926f;
        const float k = (float)sky.w / (2.0f * PI_F);
        const float rh = length(dh) * k, rv = length(dv) * k;
        const bool hmajor = rh >= rv;
        const float major = hmajor ? rh : rv, minor = hmajor ? rv : rh;
        const F3 delta = hmajor ? dh : dv;
        // 3. - 5. filtered?  tap count, filter width, level and blend
        bool filt = major > 1.0f && major < (float)sky.w;
        int n = 1, L = 0;
        float f = 0.0f;
        if (filt) {
            const float mc = minor > 1.0f ? minor : 1.0f;
            n = major <= (mc * 1.0f) * 1.5f ? 1 : major <= (mc * 2.0f) * 1.5f ? 2 : major <= (mc * 4.0f) * 1.5f ? 4 : 8;
            const float q = major / (float)n;
            const float rho = q > mc ? q : mc;
            L = (int)((f2u(rho) >> 23) & 255u) - 127;
            f = rho * u2f((uint32_t)(127 - L) << 23) - 1.0f;
            if (L < 0 || L + 1 >= pyr.levels) { filt = false; n = 1; L = 0; f = 0.0f; }   // never: 1 <= rho < sky.w <= 2^(levels - 1); no read beyond the pyramid whatever the input
        }
        // 6. the taps, in increasing t; the wave runs to its largest n
        F3 acc = f3(0.0f, 0.0f, 0.0f);
        for (int t = 0; t < n; t++) {
            F3 dt = d;
            if (filt) {
                const float s = ((float)t + 0.5f) / (float)n - 0.5f;
                dt = d + delta * s;
            }
            // cartesian_to_spherical(p.xzy), sky.wgsl:20, 32-38: sky_kernel's operations
            const float theta = bh_atan2(sqrtf(dt.x * dt.x + dt.z * dt.z), dt.y);
            const float phi = bh_atan2(dt.z, dt.x);
            float u = (phi + 2.6f * PI_F) / (2.0f * PI_F);
            float v = (PI_F - theta) / PI_F;
            u = u - truncf(u); v = v - truncf(v);
            F3 T = sample_level(sky, pyr, L, u, v);
            if (f != 0.0f) T = mix3(T, sample_level(sky, pyr, L + 1, u, v), f);
            acc = t == 0 ? T : acc + T;
        }
        // 7. the mean
        const float inv = 1.0f / (float)n;
        p = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, 1.0f);
    }
    dst[(size_t)gy * (size_t)W + (size_t)gx] = pack16(p.x, p.y, p.z, p.w);   // rgba16float target (sky.wgsl:1): round to nearest even
}

}  // namespace

int sky_pyramid_sizes(uint32_t w, uint32_t h, uint32_t* levels, uint32_t* lw, uint32_t* lh) {
    if (w == 0 || h == 0 || w > 0x80000000u || h > 0x80000000u || !levels || !lw || !lh) return BHRAY_E_INVALID;   // 2^31 is 1 after 31 halvings: 32 levels
    uint32_t n = 0;
    for (;;) {
        lw[n] = w; lh[n] = h; n++;
        if (w == 1 && h == 1) break;
        w = (uint32_t)(((uint64_t)w + 1) >> 1); h = (uint32_t)(((uint64_t)h + 1) >> 1);
    }
    *levels = n;
    return BHRAY_OK;
}

size_t sky_pyramid_layout(int w, int h, SkyPyr* out) {
    uint32_t n = 0, lw[32], lh[32];
    *out = SkyPyr{};
    if (w < 1 || h < 1 || w > 32768 || h > 32768 || sky_pyramid_sizes((uint32_t)w, (uint32_t)h, &n, lw, lh) != BHRAY_OK || n > (uint32_t)SKY_PYR_MAX_LEVELS) return 0;
    size_t texels = 0;
    for (uint32_t l = 1; l < n; l++) { out->off[l] = (uint32_t)texels; texels += (size_t)lw[l] * lh[l]; }
    out->levels = (int)n;
    return texels;
}

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_sky_pyramid_first(const TexDev& sky, uint2* dst, hipStream_t s) {
    const int dw = sky_pyr_dim(sky.w, 1), dh = sky_pyr_dim(sky.h, 1);
    const size_t n = (size_t)dw * (size_t)dh;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sky_pyramid_first_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sky, dst, dw, dh);
    return hipGetLastError();
}

hipError_t launch_sky_pyramid_next(const uint2* src, int sw, int sh, uint2* dst, hipStream_t s) {
    const int dw = sky_pyr_dim(sw, 1), dh = sky_pyr_dim(sh, 1);
    const size_t n = (size_t)dw * (size_t)dh;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sky_pyramid_next_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, sw, sh, dst, dw, dh);
    return hipGetLastError();
}

hipError_t launch_sky_filter(const TexDev& sky, const SkyPyr& pyr, const float4* src, uint2* dst, uint32_t frame_w, uint32_t frame_h, hipStream_t s) {
    if (frame_w == 0 || frame_h == 0) return hipSuccess;
    const unsigned gx = (frame_w + TILE_W - 1) / TILE_W, gy = (frame_h + TILE_H - 1) / TILE_H;
    if (gy > 65535u || pyr.levels < 1 || pyr.levels > SKY_PYR_MAX_LEVELS || (pyr.levels > 1 && !pyr.base)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sky_filter_kernel, dim3(gx, gy), dim3(256), 0, s, sky, pyr, src, dst, (int)frame_w, (int)frame_h);
    return hipGetLastError();
}

}  // namespace bhray

extern "C" int bhray_sky_pyramid_sizes(uint32_t w, uint32_t h, uint32_t* levels, uint32_t* lw, uint32_t* lh) { return bhray::sky_pyramid_sizes(w, h, levels, lw, lh); }
