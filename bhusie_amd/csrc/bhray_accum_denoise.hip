// bhray_accum_denoise.hip — the kernels of the denoised stills (bhray_accum_read_denoised): an edge-avoiding a-trous filter over the accumulation's
// colour mean, guided by the means of its still passes.  A read-time function of the sums: nothing here writes accumulation state.
//
//   denoise_prepare_kernel   one thread per pixel reads the colour sum and the pass sums the guide set needs, once, forms the means by accum_mean_kernel's operations
//                            and writes the colour mean, its (r, g, b, t) texel and up to three packed guide texels
//   denoise_atrous_kernel    one iteration at tap spacing `step`.  The pixels with equal (x mod step, y mod step) form a dense sub-image - a lattice - on which the
//                            25 taps are a plain 5 x 5 stencil, so one kernel serves all five spacings.  A block is four waves on a 32 x 8 tile of lattice pixels of
//                            one residue: it loads the tile plus a halo of 2 (36 x 12 texels) ONCE into separate float4 planes in LDS - the colour with t and the
//                            guide planes the set needs, 6912 bytes each, at most 27 648 - and every thread runs denoise_pixel over them.
//
// A 32-lane half of a wave is 32 consecutive lattice pixels of one row, so its float4 LDS reads fall on consecutive 16-byte slots of one plane and every 16-lane
// group of the read covers 16 distinct slots of the 256-byte bank row: conflict-free (one 64-byte record per texel would put the lanes 64 bytes apart: 4-way).  Each
// texel is fetched (36 * 12) / (32 * 8) = 1.7 times per iteration instead of 25.  At spacing 8 and 16 a lane's global load uses 16 of each 128-byte line; the
// residues next to it in x are the blocks next to it in the grid (the residue is the fast part of blockIdx.x), which use the rest out of L2.  The guide set is a
// kernel argument: uniform over the grid.  No atomics: a pixel has one writer.  Translation unit of its own, so that no pre-existing kernel's registers or schedule
// can move with it; compiled -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstring>
#include <vector>

#include "bhray_accum_denoise.h"

namespace bhray {
namespace {

constexpr int TILE_W = 32, TILE_H = 8, HALO = 2;                  // tile of a block (lattice pixels) and the stencil's reach
constexpr int TILE_P = TILE_W + 2 * HALO, TILE_R = TILE_H + 2 * HALO;   // pitch and rows of its LDS copy
static_assert(TILE_W * TILE_H == 256 && TILE_W == 32, "a 32-lane half of a wave is one row of the tile");

BH_HD float4 mean_of(const float4& a) {                           // accum_mean_kernel's operations
    return a.w == 0.0f ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(a.x / a.w, a.y / a.w, a.z / a.w, 1.0f);
}

__global__ __launch_bounds__(256) void denoise_prepare_kernel(const float4* __restrict__ sum, const AccumPassPlanes planes, uint32_t guides, float4* __restrict__ mean,
                                                              float4* __restrict__ ct, float4* __restrict__ g0, float4* __restrict__ g1, float4* __restrict__ g2,
                                                              uint32_t npix) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 m = mean_of(sum[p]);
    mean[p] = m;
    ct[p] = denoise_texel(m.x, m.y, m.z, m.w);
    if (guides & DENOISE_NEEDS_G0) {                              // (uniform over the grid, as the two below)
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (guides & BHRAY_PASS_COVERAGE) { const float4 c = mean_of(planes.plane[0][p]); v.x = c.x; v.y = c.y; v.z = c.z; }
        if (guides & BHRAY_PASS_GEOMETRY) v.w = mean_of(planes.plane[1][p]).x;
        g0[p] = v;
    }
    if (guides & DENOISE_NEEDS_G1) g1[p] = mean_of(planes.plane[2][p]);
    if (guides & DENOISE_NEEDS_G2) g2[p] = mean_of(planes.plane[3][p]);
}

// denoise_pixel's view of a block's LDS planes around the thread's texel
struct TileTaps {
    const float4* ct_; const float4* g0_; const float4* g1_; const float4* g2_;
    int at;                                                       // the thread's own texel in the planes
    __device__ __forceinline__ float4 ct(int a, int b) const { return ct_[at + b * TILE_P + a]; }
    __device__ __forceinline__ float4 g0(int a, int b) const { return g0_[at + b * TILE_P + a]; }
    __device__ __forceinline__ float4 g1(int a, int b) const { return g1_[at + b * TILE_P + a]; }
    __device__ __forceinline__ float4 g2(int a, int b) const { return g2_[at + b * TILE_P + a]; }
};

// blockIdx.x = tile_x * step + rx, blockIdx.y = tile_y * step + ry: lattice pixel (lx, ly) of residue (rx, ry) is frame pixel (rx + lx * step, ry + ly * step)
__global__ __launch_bounds__(256) void denoise_atrous_kernel(const DenoiseRule rule, const float4* __restrict__ src, const float4* __restrict__ g0,
                                                             const float4* __restrict__ g1, const float4* __restrict__ g2, const float4* __restrict__ mean,
                                                             float4* __restrict__ dst, uint2* __restrict__ out16, int W, int H, int step, int last) {
    __shared__ float4 s_ct[TILE_R * TILE_P], s_g0[TILE_R * TILE_P], s_g1[TILE_R * TILE_P], s_g2[TILE_R * TILE_P];
    const int tid = (int)threadIdx.x;
    const int tile_x = (int)blockIdx.x / step, rx = (int)blockIdx.x - tile_x * step;
    const int tile_y = (int)blockIdx.y / step, ry = (int)blockIdx.y - tile_y * step;
    const int bx = tile_x * TILE_W, by = tile_y * TILE_H;         // the tile's first lattice pixel
    const bool need0 = (rule.guides & DENOISE_NEEDS_G0) != 0, need1 = (rule.guides & DENOISE_NEEDS_G1) != 0, need2 = (rule.guides & DENOISE_NEEDS_G2) != 0;
    for (int i = tid; i < TILE_R * TILE_P; i += 256) {            // (a thread outside the frame still loads and meets the barrier)
        const int ly = i / TILE_P, lx = i - ly * TILE_P;
        const int x = rx + (bx + lx - HALO) * step, y = ry + (by + ly - HALO) * step;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = (size_t)y * (size_t)W + (size_t)x;
            s_ct[i] = src[q];
            if (need0) s_g0[i] = g0[q];
            if (need1) s_g1[i] = g1[q];
            if (need2) s_g2[i] = g2[q];
        } else {
            s_ct[i] = make_float4(0.0f, 0.0f, 0.0f, u2f(DENOISE_INVALID_BITS));   // outside the frame: no tap; its guide texels are never read
        }
    }
    __syncthreads();
    const int tx = tid & (TILE_W - 1), ty = tid >> 5;
    const int gx = rx + (bx + tx) * step, gy = ry + (by + ty) * step;
    if (gx >= W || gy >= H) return;
    TileTaps taps;
    taps.ct_ = s_ct; taps.g0_ = s_g0; taps.g1_ = s_g1; taps.g2_ = s_g2;
    taps.at = (ty + HALO) * TILE_P + tx + HALO;
    float4 v = denoise_pixel(rule, taps);
    const size_t p = (size_t)gy * (size_t)W + (size_t)gx;
    if (last) {
        v.w = denoise_valid_t(s_ct[taps.at].w) ? 1.0f : mean[p].w;   // alpha is kept: 1 for a pixel that was valid, C_0's otherwise
        if (out16) {                                              // accum_mean_kernel's conversion
            const uint32_t lo = (uint32_t)__half_as_ushort(__float2half_rn(v.x)) | ((uint32_t)__half_as_ushort(__float2half_rn(v.y)) << 16);
            const uint32_t hi = (uint32_t)__half_as_ushort(__float2half_rn(v.z)) | ((uint32_t)__half_as_ushort(__float2half_rn(v.w)) << 16);
            out16[p] = make_uint2(lo, hi);
        }
    }
    dst[p] = v;
}

bool sigma_ok(float s) { return std::isfinite(s) && s > 0.0f; }

// denoise_pixel's view of whole images on the host
struct ImageTaps {
    const float4* ct_; const float4* g0_; const float4* g1_; const float4* g2_;
    int W, H, x, y, step;
    size_t at(int a, int b) const { return (size_t)(y + b * step) * (size_t)W + (size_t)(x + a * step); }
    bool in(int a, int b) const { const int xx = x + a * step, yy = y + b * step; return xx >= 0 && xx < W && yy >= 0 && yy < H; }
    float4 ct(int a, int b) const { return in(a, b) ? ct_[at(a, b)] : make_float4(0.0f, 0.0f, 0.0f, u2f(DENOISE_INVALID_BITS)); }
    float4 g0(int a, int b) const { return g0_[at(a, b)]; }       // (asked only behind a valid ct: inside the frame)
    float4 g1(int a, int b) const { return g1_[at(a, b)]; }
    float4 g2(int a, int b) const { return g2_[at(a, b)]; }
};

}  // namespace

const char* still_denoise_error(const bhray_still_denoise* p, uint32_t set) {
    if (!p) return nullptr;                                       // NULL: the defaults
    if (p->struct_size != sizeof(bhray_still_denoise)) return "struct_size is not sizeof(bhray_still_denoise)";
    if (p->iterations < 1 || p->iterations > BHRAY_DENOISE_MAX_ITERATIONS) return "iterations must be 1 .. 5";
    if (p->guides & ~set) return "guides names a pass that is not in the set";
    if (!sigma_ok(p->sigma_colour) || !sigma_ok(p->sigma_coverage) || !sigma_ok(p->sigma_closest) || !sigma_ok(p->sigma_position) || !sigma_ok(p->sigma_escape))
        return "every sigma must be finite and > 0";
    return nullptr;
}

void denoise_rule_fill(DenoiseRule& r, const bhray_still_denoise* p, uint32_t set) {
    bhray_still_denoise d;
    if (!p) { bhray_still_denoise_default(&d); p = &d; }
    r.guides = p->guides ? p->guides : set;
    r.s2_colour = p->sigma_colour * p->sigma_colour;
    r.s2_coverage = p->sigma_coverage * p->sigma_coverage;
    r.s2_closest = p->sigma_closest * p->sigma_closest;
    r.s2_position = p->sigma_position * p->sigma_position;
    r.s2_escape = p->sigma_escape * p->sigma_escape;
}

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_denoise_prepare(const float4* sum, const AccumPassPlanes& planes, uint32_t guides, float4* mean, float4* ct, float4* g0, float4* g1, float4* g2,
                                  uint32_t npix, hipStream_t s) {
    if (npix == 0) return hipSuccess;
    if (!sum || !mean || !ct || guides == 0 || (guides & ~(uint32_t)BHRAY_PASS_ALL)) return hipErrorInvalidValue;
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) if (((guides >> b) & 1u) && !planes.plane[b]) return hipErrorInvalidValue;
    if (((guides & DENOISE_NEEDS_G0) && !g0) || ((guides & DENOISE_NEEDS_G1) && !g1) || ((guides & DENOISE_NEEDS_G2) && !g2)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, sum, planes, guides, mean, ct, g0, g1, g2, npix);
    return hipGetLastError();
}

hipError_t launch_denoise_atrous(const DenoiseRule& rule, const float4* src, const float4* g0, const float4* g1, const float4* g2, const float4* mean, float4* dst,
                                 uint2* out16, uint32_t frame_w, uint32_t frame_h, uint32_t step, bool last, hipStream_t s) {
    if (frame_w == 0 || frame_h == 0) return hipSuccess;
    if (!src || !dst || src == dst || !mean || rule.guides == 0 || (rule.guides & ~(uint32_t)BHRAY_PASS_ALL) || frame_w > (1u << 24) || frame_h > (1u << 24)) return hipErrorInvalidValue;
    if (step != 1 && step != 2 && step != 4 && step != 8 && step != 16) return hipErrorInvalidValue;
    if (((rule.guides & DENOISE_NEEDS_G0) && !g0) || ((rule.guides & DENOISE_NEEDS_G1) && !g1) || ((rule.guides & DENOISE_NEEDS_G2) && !g2)) return hipErrorInvalidValue;
    const uint32_t lw = (frame_w + step - 1) / step, lh = (frame_h + step - 1) / step;   // the largest lattice
    const uint32_t gx = ((lw + TILE_W - 1) / TILE_W) * step, gy = ((lh + TILE_H - 1) / TILE_H) * step;
    if (gy > 65535u) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(denoise_atrous_kernel, dim3(gx, gy), dim3(256), 0, s, rule, src, g0, g1, g2, mean, dst, out16, (int)frame_w, (int)frame_h, (int)step, last ? 1 : 0);
    return hipGetLastError();
}

}  // namespace bhray

// How the defaults were chosen is written down in DESIGN.md §28.
extern "C" void bhray_still_denoise_default(bhray_still_denoise* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof(bhray_still_denoise);
    p->iterations = 2;
    p->guides = 0;
    p->sigma_colour = 0.5f;
    p->sigma_coverage = 1.0f;
    p->sigma_closest = 4.0f;
    p->sigma_position = 8.0f;
    p->sigma_escape = 1.0f;
}

// pure host arithmetic through denoise_texel and denoise_pixel - no ctx, no device
extern "C" int bhray_accum_denoise_host(const float* colour, const float* const guide[4], uint32_t w, uint32_t h, const bhray_still_denoise* p, float* out) {
    using namespace bhray;
    if (!colour || !guide || !out || w == 0 || h == 0 || w > (1u << 24) || h > (1u << 24)) return BHRAY_E_INVALID;
    uint32_t set = 0;
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) if (guide[b]) set |= 1u << b;
    bhray_still_denoise defaults;
    if (!p) { bhray_still_denoise_default(&defaults); p = &defaults; }
    if (set == 0 || still_denoise_error(p, set)) return BHRAY_E_INVALID;
    DenoiseRule rule;
    denoise_rule_fill(rule, p, set);
    const uint32_t iterations = p->iterations;
    const size_t npix = (size_t)w * (size_t)h;
    const float4* C = reinterpret_cast<const float4*>(colour);
    std::vector<float4> ct[2], g[3];
    ct[0].resize(npix); ct[1].resize(npix);
    if (rule.guides & DENOISE_NEEDS_G0) g[0].assign(npix, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    if (rule.guides & DENOISE_NEEDS_G1) g[1].resize(npix);
    if (rule.guides & DENOISE_NEEDS_G2) g[2].resize(npix);
    for (size_t i = 0; i < npix; i++) {
        ct[0][i] = denoise_texel(C[i].x, C[i].y, C[i].z, C[i].w);
        if (rule.guides & BHRAY_PASS_COVERAGE) { g[0][i].x = guide[0][4 * i]; g[0][i].y = guide[0][4 * i + 1]; g[0][i].z = guide[0][4 * i + 2]; }
        if (rule.guides & BHRAY_PASS_GEOMETRY) g[0][i].w = guide[1][4 * i];
        if (rule.guides & BHRAY_PASS_POSITION) g[1][i] = make_float4(guide[2][4 * i], guide[2][4 * i + 1], guide[2][4 * i + 2], 0.0f);
        if (rule.guides & BHRAY_PASS_ESCAPE) g[2][i] = make_float4(guide[3][4 * i], guide[3][4 * i + 1], guide[3][4 * i + 2], 0.0f);
    }
    for (uint32_t it = 0; it < iterations; it++) {
        ImageTaps taps;
        taps.ct_ = ct[it & 1].data(); taps.g0_ = g[0].data(); taps.g1_ = g[1].data(); taps.g2_ = g[2].data();
        taps.W = (int)w; taps.H = (int)h; taps.step = 1 << it;
        float4* dst = ct[(it + 1) & 1].data();
        for (taps.y = 0; taps.y < (int)h; taps.y++)
            for (taps.x = 0; taps.x < (int)w; taps.x++) dst[(size_t)taps.y * w + (size_t)taps.x] = denoise_pixel(rule, taps);
    }
    const float4* R = ct[iterations & 1].data();
    for (size_t i = 0; i < npix; i++) { out[4 * i] = R[i].x; out[4 * i + 1] = R[i].y; out[4 * i + 2] = R[i].z; out[4 * i + 3] = C[i].w; }   // alpha is kept
    return BHRAY_OK;
}
