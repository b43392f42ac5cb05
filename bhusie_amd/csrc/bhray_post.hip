// bhray_post.hip — gfx950 kernels of the display pass: the reference's GPU frame after the sky pass
// (src/renderer/mod.rs:209-324 wiring, 425-431 dispatch):
//
//   bloom_down x5   bloom_down.wgsl   13 taps of the previous level, NEAREST (min filter, source ~2x the target)
//   bloom_up   x4   bloom_up.wgsl     9 bilinear taps of the previous level (mag filter Linear)
//   final_kernel    bloom_up.wgsl (last up pass) + mix.wgsl + hdr.wgsl: per pixel at 1:1, fused; the three Rgba16Float
//                   roundings (bloom -> fp16, mix -> fp16, ACES -> fp16) are kept, so it is the same bits as three passes
//   fxaa_kernel     fxaa.wgsl into the Rgba8UnormSrgb target: linear -> sRGB by an exact threshold table
//
// Every image between the passes is RGBA16F (8-byte pixels, loaded and stored as uint2).  One thread per target pixel, 256-thread
// blocks.  Operation order is the WGSL text's, in binary32, without contraction (the Makefile's -ffp-contract=off): DESIGN.md §10.
#include <hip/hip_fp16.h>
#include <math.h>
#include <string.h>

#include "bhray_internal.h"
#include "bhray_math.h"

namespace bhray {

namespace {

__device__ __forceinline__ float h2f(uint32_t bits) { return __half2float(__ushort_as_half((unsigned short)(bits & 0xffffu))); }
__device__ __forceinline__ uint32_t f2h(float f) { return (uint32_t)__half_as_ushort(__float2half_rn(f)); }
__device__ __forceinline__ float4 unpack16(uint2 p) { return make_float4(h2f(p.x), h2f(p.x >> 16), h2f(p.y), h2f(p.y >> 16)); }
__device__ __forceinline__ uint2 pack16(float4 v) { return make_uint2(f2h(v.x) | (f2h(v.y) << 16), f2h(v.z) | (f2h(v.w) << 16)); }

struct Img { const uint2* __restrict__ p; int w, h; };

__device__ __forceinline__ float4 texel16(const Img& t, int x, int y) { return unpack16(t.p[(size_t)y * (size_t)t.w + (size_t)x]); }

// The fragment's texture coordinate (quad.rs: v = 0 on the top row): pixel (x, y) of a w x h target
__device__ __forceinline__ float frag_u(int x, int w) { return ((float)x + 0.5f) / (float)w; }

// min filter Nearest: texel floor(u * n), clamped to the edge
__device__ __forceinline__ int nearest_index(float u, int n) {
    const float x = floorf(u * (float)n);
    if (!(x >= 0.0f)) return 0;
    if (x >= (float)(n - 1)) return n - 1;
    return (int)x;
}

// mag filter Linear, clamp to edge: the project's bilinear convention (bhray_kernels.hip `unit_coord`), with the integer texel offset of
// textureSampleLevel(..., offset) added to the texel coordinate after the -0.5
__device__ __forceinline__ float lin_coord(float u, int n, int off, int& i0, int& i1) {
    float x = u * (float)n - 0.5f;
    x = x + (float)off;
    if (!(x >= -1.0f)) x = -1.0f;
    if (x > (float)n) x = (float)n;
    const float fl = floorf(x);
    int a = (int)fl, b = a + 1;
    a = a < 0 ? 0 : a; a = a > n - 1 ? n - 1 : a;
    b = b < 0 ? 0 : b; b = b > n - 1 ? n - 1 : b;
    i0 = a; i1 = b;
    return x - fl;
}
__device__ __forceinline__ float4 bilinear16(const Img& t, float u, float v, int ox = 0, int oy = 0) {
    int x0, x1, y0, y1;
    const float fx = lin_coord(u, t.w, ox, x0, x1);
    const float fy = lin_coord(v, t.h, oy, y0, y1);
    const float4 a = texel16(t, x0, y0), b = texel16(t, x1, y0), c = texel16(t, x0, y1), d = texel16(t, x1, y1);
    float4 r;
    r.x = mix_(mix_(a.x, b.x, fx), mix_(c.x, d.x, fx), fy);
    r.y = mix_(mix_(a.y, b.y, fx), mix_(c.y, d.y, fx), fy);
    r.z = mix_(mix_(a.z, b.z, fx), mix_(c.z, d.z, fx), fy);
    r.w = mix_(mix_(a.w, b.w, fx), mix_(c.w, d.w, fx), fy);
    return r;
}

__device__ __forceinline__ F3 rgb(float4 v) { return f3(v.x, v.y, v.z); }

// bloom_down.wgsl:fs_main
__device__ __forceinline__ F3 bloom_down_px(const Img& s, int x, int y, int tw, int th) {
    const float u = frag_u(x, tw), v = frag_u(y, th);
    const float sx = 1.0f / (float)s.w, sy = 1.0f / (float)s.h;          // src_texel_size
    const float x2 = 2.0f * sx, y2 = 2.0f * sy;
    const int cm2 = nearest_index(u - x2, s.w), c0 = nearest_index(u, s.w), cp2 = nearest_index(u + x2, s.w);
    const int cm1 = nearest_index(u - sx, s.w), cp1 = nearest_index(u + sx, s.w);
    const int rp2 = nearest_index(v + y2, s.h), r0 = nearest_index(v, s.h), rm2 = nearest_index(v - y2, s.h);
    const int rp1 = nearest_index(v + sy, s.h), rm1 = nearest_index(v - sy, s.h);
    const F3 a = rgb(texel16(s, cm2, rp2)), b = rgb(texel16(s, c0, rp2)), c = rgb(texel16(s, cp2, rp2));
    const F3 d = rgb(texel16(s, cm2, r0)),  e = rgb(texel16(s, c0, r0)),  f = rgb(texel16(s, cp2, r0));
    const F3 g = rgb(texel16(s, cm2, rm2)), h = rgb(texel16(s, c0, rm2)), i = rgb(texel16(s, cp2, rm2));
    const F3 j = rgb(texel16(s, cm1, rp1)), k = rgb(texel16(s, cp1, rp1));
    const F3 l = rgb(texel16(s, cm1, rm1)), m = rgb(texel16(s, cp1, rm1));
    F3 ds = e * 0.125f;
    ds = ds + (((a + c) + g) + i) * 0.03125f;
    ds = ds + (((b + d) + f) + h) * 0.0625f;
    ds = ds + (((j + k) + l) + m) * 0.125f;
    return ds;
}

// bloom_up.wgsl:fs_main (the taps' offsets are 0.005 in uv, not texels)
__device__ __forceinline__ F3 bloom_up_px(const Img& s, int x, int y, int tw, int th) {
    const float u = frag_u(x, tw), v = frag_u(y, th);
    const float o = 0.005f;
    const float um = u - o, up = u + o, vp = v + o, vm = v - o;
    const F3 a = rgb(bilinear16(s, um, vp)), b = rgb(bilinear16(s, u, vp)), c = rgb(bilinear16(s, up, vp));
    const F3 d = rgb(bilinear16(s, um, v)),  e = rgb(bilinear16(s, u, v)),  f = rgb(bilinear16(s, up, v));
    const F3 g = rgb(bilinear16(s, um, vm)), h = rgb(bilinear16(s, u, vm)), i = rgb(bilinear16(s, up, vm));
    F3 us = e * 4.0f;
    us = us + (((b + d) + f) + h) * 2.0f;
    us = us + (((a + c) + g) + i);
    us = us * (1.0f / 16.0f);
    return us;
}

__global__ __launch_bounds__(256) void bloom_kernel(Img src, uint2* __restrict__ dst, int tw, int th, int up) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= tw * th) return;
    const int x = idx % tw, y = idx / tw;
    const F3 r = up ? bloom_up_px(src, x, y, tw, th) : bloom_down_px(src, x, y, tw, th);
    dst[idx] = pack16(make_float4(r.x, r.y, r.z, 1.0f));
}

// hdr.wgsl:aces_tone_map.  mat3x3 * v in WGSL's column-major order ((c0 x + c1 y) + c2 z); clamp = min(max(x, 0), 1) with maxNum /
// minNum semantics (NaN -> 0, as v_max_f32 / v_min_f32)
__device__ __forceinline__ float aces1(float v) {
    const float a = v * (v + 0.0245786f) - 0.000090537f;
    const float b = v * (0.983729f * v + 0.4329510f) + 0.238081f;
    return a / b;
}
__device__ __forceinline__ F3 aces(F3 h) {
    const F3 v = f3((0.59719f * h.x + 0.35458f * h.y) + 0.04823f * h.z,
                    (0.07600f * h.x + 0.90834f * h.y) + 0.01566f * h.z,
                    (0.02840f * h.x + 0.13383f * h.y) + 0.83777f * h.z);
    const F3 q = f3(aces1(v.x), aces1(v.y), aces1(v.z));
    const F3 m = f3((1.60475f * q.x + -0.53108f * q.y) + -0.07367f * q.z,
                    (-0.10208f * q.x + 1.10813f * q.y) + -0.00605f * q.z,
                    (-0.00327f * q.x + -0.07276f * q.y) + 1.07602f * q.z);
    return f3(fminf(fmaxf(m.x, 0.0f), 1.0f), fminf(fmaxf(m.y, 0.0f), 1.0f), fminf(fmaxf(m.z, 0.0f), 1.0f));
}

// The last bloom-up pass, mix.wgsl and hdr.wgsl at W x H, one pixel each: the up pass's taps, then this pixel of the sky image
__global__ __launch_bounds__(256) void final_kernel(Img src, const uint2* __restrict__ sky, uint2* __restrict__ dst, int w, int h, float ratio) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= w * h) return;
    const int x = idx % w, y = idx / w;
    const float4 s = unpack16(sky[idx]);
    const F3 b3 = bloom_up_px(src, x, y, w, h);
    const float4 bl = unpack16(pack16(make_float4(b3.x, b3.y, b3.z, 1.0f)));      // the bloom target is Rgba16Float
    const float r1 = 1.0f - ratio;                                                 // mix.wgsl: r * t_input_1 (sky) + (1 - r) * t_input_2 (bloom)
    const float4 mx = unpack16(pack16(make_float4(ratio * s.x + r1 * bl.x, ratio * s.y + r1 * bl.y, ratio * s.z + r1 * bl.z, ratio * s.w + r1 * bl.w)));
    const F3 t = aces(f3(mx.x, mx.y, mx.z));
    dst[idx] = pack16(make_float4(t.x, t.y, t.z, mx.w));                           // hdr.wgsl keeps the mixed alpha
}

__device__ __forceinline__ float luma(float4 c) { return sqrtf((c.x * 0.299f + c.y * 0.587f) + c.z * 0.114f); }   // rgb2luma

__device__ __forceinline__ float quality(int q) {
    switch (q) {
        default: return 1.0f;
        case 5: return 1.5f;
        case 6: case 7: case 8: case 9: return 2.0f;
        case 10: return 4.0f;
        case 11: return 8.0f;
    }
}

// Rgba8UnormSrgb store: the number of decision thresholds <= v (255 increasing thresholds in LDS; NaN -> 0)
__device__ __forceinline__ uint32_t srgb_byte(const float* thr, float v) {
    int lo = 0;
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1)
        if (lo + step <= 255 && thr[lo + step - 1] <= v) lo += step;
    return (uint32_t)lo;
}
__device__ __forceinline__ uint32_t unorm_byte(float a) {
    if (!(a > 0.0f)) return 0u;
    if (a >= 1.0f) return 255u;
    return (uint32_t)rintf(a * 255.0f);
}

__global__ __launch_bounds__(256) void fxaa_kernel(Img t, uint32_t* __restrict__ dst, PostArgs P) {
    __shared__ float thr[256];
    thr[threadIdx.x] = threadIdx.x < 255 ? P.srgb_thr[threadIdx.x] : 0.0f;
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= t.w * t.h) return;
    const int px = idx % t.w, py = idx / t.w;
    const float isx = 1.0f / (float)t.w, isy = 1.0f / (float)t.h;                  // inverseScreenSize
    const float tcx = ((float)px + 0.5f) * isx, tcy = ((float)py + 0.5f) * isy;    // in.position.xy * inverseScreenSize

    const float4 centerSample = bilinear16(t, tcx, tcy);
    const float lumaCenter = luma(centerSample);
    const float lumaDown = luma(bilinear16(t, tcx, tcy, 0, -1));
    const float lumaUp = luma(bilinear16(t, tcx, tcy, 0, 1));
    const float lumaLeft = luma(bilinear16(t, tcx, tcy, -1, 0));
    const float lumaRight = luma(bilinear16(t, tcx, tcy, 1, 0));
    const float lumaMin = min_(lumaCenter, min_(min_(lumaDown, lumaUp), min_(lumaLeft, lumaRight)));
    const float lumaMax = max_(lumaCenter, max_(max_(lumaDown, lumaUp), max_(lumaLeft, lumaRight)));
    const float lumaRange = lumaMax - lumaMin;

    float4 outc;
    if (lumaRange < max_(P.edge_min, lumaMax * P.edge_max)) {
        outc = centerSample;
    } else {
        const float lumaDownLeft = luma(bilinear16(t, tcx, tcy, -1, -1));
        const float lumaUpRight = luma(bilinear16(t, tcx, tcy, 1, 1));
        const float lumaUpLeft = luma(bilinear16(t, tcx, tcy, -1, 1));
        const float lumaDownRight = luma(bilinear16(t, tcx, tcy, 1, -1));
        const float lumaDownUp = lumaDown + lumaUp;
        const float lumaLeftRight = lumaLeft + lumaRight;
        const float lumaLeftCorners = lumaDownLeft + lumaUpLeft;
        const float lumaDownCorners = lumaDownLeft + lumaDownRight;
        const float lumaRightCorners = lumaDownRight + lumaUpRight;
        const float lumaUpCorners = lumaUpRight + lumaUpLeft;
        const float edgeHorizontal = (fabsf(-2.0f * lumaLeft + lumaLeftCorners) + fabsf(-2.0f * lumaCenter + lumaDownUp) * 2.0f) + fabsf(-2.0f * lumaRight + lumaRightCorners);
        const float edgeVertical = (fabsf(-2.0f * lumaUp + lumaUpCorners) + fabsf(-2.0f * lumaCenter + lumaLeftRight) * 2.0f) + fabsf(-2.0f * lumaDown + lumaDownCorners);
        const bool isHorizontal = edgeHorizontal >= edgeVertical;
        float stepLength = isHorizontal ? isy : isx;
        const float luma1 = isHorizontal ? lumaDown : lumaLeft;
        const float luma2 = isHorizontal ? lumaUp : lumaRight;
        const float gradient1 = luma1 - lumaCenter, gradient2 = luma2 - lumaCenter;
        const bool is1Steepest = fabsf(gradient1) >= fabsf(gradient2);
        const float gradientScaled = 0.25f * max_(fabsf(gradient1), fabsf(gradient2));
        float lumaLocalAverage;
        if (is1Steepest) { stepLength = -stepLength; lumaLocalAverage = 0.5f * (luma1 + lumaCenter); }
        else lumaLocalAverage = 0.5f * (luma2 + lumaCenter);
        float cux = tcx, cuy = tcy, ofx = 0.0f, ofy = 0.0f;
        if (isHorizontal) { cuy = cuy + stepLength * 0.5f; ofx = isx; }
        else { cux = cux + stepLength * 0.5f; ofy = isy; }
        float u1x = cux - ofx, u1y = cuy - ofy, u2x = cux + ofx, u2y = cuy + ofy;
        float lumaEnd1 = luma(bilinear16(t, u1x, u1y)) - lumaLocalAverage;
        float lumaEnd2 = luma(bilinear16(t, u2x, u2y)) - lumaLocalAverage;
        bool reached1 = fabsf(lumaEnd1) >= gradientScaled;
        bool reached2 = fabsf(lumaEnd2) >= gradientScaled;
        bool reachedBoth = reached1 && reached2;
        // fxaa.wgsl:131-132: uv1 = select(uv1 - offset, uv1, reached1); uv2 = select(uv2 - offset, uv2, reached2) - BOTH ends step by
        // MINUS offset here (the textbook FXAA moves end 2 by +offset; the reference's text does not, and the text is the contract)
        if (!reached1) { u1x = u1x - ofx; u1y = u1y - ofy; }
        if (!reached2) { u2x = u2x - ofx; u2y = u2y - ofy; }
        if (!reachedBoth) {
            for (int i = 2; i < P.iterations; i++) {
                if (!reached1) lumaEnd1 = luma(bilinear16(t, u1x, u1y)) - lumaLocalAverage;
                if (!reached2) lumaEnd2 = luma(bilinear16(t, u2x, u2y)) - lumaLocalAverage;
                reached1 = fabsf(lumaEnd1) >= gradientScaled;
                reached2 = fabsf(lumaEnd2) >= gradientScaled;
                reachedBoth = reached1 && reached2;
                const float q = quality(i);
                if (!reached1) { u1x = u1x - ofx * q; u1y = u1y - ofy * q; }
                if (!reached2) { u2x = u2x + ofx * q; u2y = u2y + ofy * q; }
                if (reachedBoth) break;
            }
        }
        const float distance1 = isHorizontal ? tcx - u1x : tcy - u1y;
        const float distance2 = isHorizontal ? u2x - tcx : u2y - tcy;
        const bool isDirection1 = distance1 < distance2;
        const float distanceFinal = min_(distance1, distance2);
        const float edgeThickness = distance1 + distance2;
        const bool isLumaCenterSmaller = lumaCenter < lumaLocalAverage;
        const bool correctVariation1 = (lumaEnd1 < 0.0f) != isLumaCenterSmaller;
        const bool correctVariation2 = (lumaEnd2 < 0.0f) != isLumaCenterSmaller;
        const bool correctVariation = isDirection1 ? correctVariation1 : correctVariation2;
        const float pixelOffset = -distanceFinal / edgeThickness + 0.5f;
        float finalOffset = correctVariation ? pixelOffset : 0.0f;
        const float lumaAverage = P.one_twelfth * (((2.0f * (lumaDownUp + lumaLeftRight)) + lumaLeftCorners) + lumaRightCorners);
        const float subPixelOffset1 = fminf(fmaxf(fabsf(lumaAverage - lumaCenter) / lumaRange, 0.0f), 1.0f);
        const float subPixelOffset2 = ((-2.0f * subPixelOffset1 + 3.0f) * subPixelOffset1) * subPixelOffset1;
        const float subPixelOffsetFinal = (subPixelOffset2 * subPixelOffset2) * P.subpix;
        finalOffset = max_(finalOffset, subPixelOffsetFinal);
        float fux = tcx, fuy = tcy;
        if (isHorizontal) fuy = fuy + finalOffset * stepLength;
        else fux = fux + finalOffset * stepLength;
        const float4 fc = bilinear16(t, fux, fuy);
        outc = make_float4(fc.x, fc.y, fc.z, centerSample.w);
    }
    dst[idx] = srgb_byte(thr, outc.x) | (srgb_byte(thr, outc.y) << 8) | (srgb_byte(thr, outc.z) << 16) | (unorm_byte(outc.w) << 24);
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// rule 1 of DESIGN.md §10: the reference's f32 `current_res` halved five times, then doubled five times; every target is (u32) of the float
int bloom_sizes(uint32_t fw, uint32_t fh, uint32_t w[BHRAY_BLOOM_LEVELS], uint32_t h[BHRAY_BLOOM_LEVELS]) {
    float cw = (float)fw, ch = (float)fh;
    for (int i = 0; i < BHRAY_BLOOM_LEVELS; i++) {
        if (i < BHRAY_BLOOM_LEVELS / 2) { cw = cw / 2.0f; ch = ch / 2.0f; } else { cw = cw * 2.0f; ch = ch * 2.0f; }
        w[i] = (uint32_t)cw; h[i] = (uint32_t)ch;
        if (w[i] == 0 || h[i] == 0) return BHRAY_E_INVALID;
    }
    return BHRAY_OK;
}

size_t display_scratch_bytes(uint32_t fw, uint32_t fh) {
    uint32_t w[BHRAY_BLOOM_LEVELS], h[BHRAY_BLOOM_LEVELS];
    if (bloom_sizes(fw, fh, w, h)) return 0;
    size_t n = 0;
    for (int i = 0; i + 1 < BHRAY_BLOOM_LEVELS; i++) n += (size_t)w[i] * h[i];
    return (n + (size_t)fw * fh) * sizeof(uint2);          // the nine intermediate bloom levels, then the tone-mapped image
}

// the decision thresholds of the sRGB encoding: byte >= k <=> v >= srgb_decode((k - 0.5) / 255), formed in double and rounded UP to f32 (the
// smallest f32 not below the threshold): a value equal to a threshold that had been rounded down lies below the real one and takes byte k - 1
static void srgb_thresholds(float* t) {
    for (int k = 1; k <= 255; k++) {
        const double c = ((double)k - 0.5) / 255.0;
        const double lin = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
        float f = (float)lin;
        if ((double)f < lin) f = nextafterf(f, INFINITY);
        t[k - 1] = f;
    }
}

// fxaa_kernel's arguments for one uniform block
static PostArgs post_args(const bhray_fxaa_details& fx) {
    static PostArgs base = [] { PostArgs a; memset(&a, 0, sizeof a); srgb_thresholds(a.srgb_thr); a.one_twelfth = (float)(1.0 / 12.0); return a; }();
    PostArgs P = base;
    P.edge_min = fx.edge_threshold_min; P.edge_max = fx.edge_threshold_max; P.iterations = fx.iterations; P.subpix = fx.subpixel_quality;
    return P;
}

hipError_t launch_fxaa(const uint2* tone, uint32_t* dst_rgba8, uint32_t fw, uint32_t fh, const bhray_fxaa_details& fx, hipStream_t s) {
    uint32_t w[BHRAY_BLOOM_LEVELS], h[BHRAY_BLOOM_LEVELS];
    if (bloom_sizes(fw, fh, w, h)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fxaa_kernel, dim3(blocks_for((size_t)fw * fh)), dim3(256), 0, s, Img{tone, (int)fw, (int)fh}, dst_rgba8, post_args(fx));
    return hipGetLastError();
}

hipError_t launch_display(const uint2* sky, uint2* scratch, uint32_t* dst_rgba8, uint32_t fw, uint32_t fh,
                          const bhray_fxaa_details& fx, const bhray_mix_details& mx, hipStream_t s) {
    uint32_t w[BHRAY_BLOOM_LEVELS], h[BHRAY_BLOOM_LEVELS];
    if (bloom_sizes(fw, fh, w, h)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    Img src{sky, (int)fw, (int)fh};
    uint2* level = scratch;
    for (int i = 0; i + 1 < BHRAY_BLOOM_LEVELS; i++) {
        const size_t n = (size_t)w[i] * h[i];
        hipLaunchKernelGGL(bloom_kernel, dim3(blocks_for(n)), dim3(256), 0, s, src, level, (int)w[i], (int)h[i], i >= BHRAY_BLOOM_LEVELS / 2 ? 1 : 0);
        src = Img{level, (int)w[i], (int)h[i]};
        level += n;
    }
    uint2* tone = level;
    const size_t npix = (size_t)fw * fh;
    hipLaunchKernelGGL(final_kernel, dim3(blocks_for(npix)), dim3(256), 0, s, src, sky, tone, (int)fw, (int)fh, mx.mix_ratio);
    hipLaunchKernelGGL(fxaa_kernel, dim3(blocks_for(npix)), dim3(256), 0, s, Img{tone, (int)fw, (int)fh}, dst_rgba8, post_args(fx));
    return hipGetLastError();
}

}  // namespace bhray

extern "C" {

int bhray_bloom_sizes(uint32_t frame_w, uint32_t frame_h, uint32_t w[10], uint32_t h[10]) {
    if (!w || !h) return BHRAY_E_INVALID;
    return bhray::bloom_sizes(frame_w, frame_h, w, h);
}

int bhray_post_defaults(bhray_fxaa_details* fxaa, bhray_mix_details* mix) {
    if (!fxaa && !mix) return BHRAY_E_INVALID;
    // Renderer::render uploads these every frame (mod.rs:375; fxaa_pipline.rs: EdgeThresholdMin / Max::Ultra; mod.rs:258-260)
    if (fxaa) { fxaa->edge_threshold_min = 0.0156f; fxaa->edge_threshold_max = 0.063f; fxaa->iterations = 12; fxaa->subpixel_quality = 0.75f; }
    if (mix) mix->mix_ratio = 0.7f;
    return BHRAY_OK;
}

}  // extern "C"
