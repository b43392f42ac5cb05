// bhray_stars.hip — the kernel of the point-star pass (bhray_set_stars), the catalogue's index build and the host form of the pass.
//
//   star_kernel   behind the sky pass: every direction pixel whose four corners are valid receives the flux of the catalogue stars inside its footprint over the
//                 footprint's solid angle, added into the RGBA16F sky image in place
//
// A stencil over the RGBA32F frame plus gathers from the catalogue, after sky_filter_kernel (§19).  A block is four waves on a 64 x 4 pixel tile; the 66 x 6 frame
// texels around it go into LDS (6336 bytes), and the 65 x 5 corners of the tile's pixels are formed ONCE per block into LDS (5200 bytes), validity in .w: a corner has
// one value whoever reads it, which is what makes neighbouring footprints tile the sky.  (Neighbouring blocks form their shared corners from the same four texels by
// the same operations, so the value is the same there too.)  Then one per-lane loop over faces, cells and stars - star_pixel of bhray_stars.h, the function the host
// form runs too; the wave runs to its busiest lane.  Every loop is bounded: 6 faces, at most BHRAY_STARS_MAX_CELLS cells, the cell's own count.  Every read is inside
// an allocation whatever the frame holds: cell coordinates are clamped to [0, G - 1] before they index the prefix array, whose entries are at most n.
// Only pixels that accepted a star read and write the sky image.  Translation unit of its own, so that no pre-existing kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <math.h>
#include <string.h>

#include "../../include/bhray_diag.h"
#include "bhray_stars.h"

namespace bhray {
namespace {

constexpr int TILE_W = 64, TILE_H = 4, TILE_P = TILE_W + 2, CORN_P = TILE_W + 1;

__device__ __forceinline__ float h2f(uint32_t bits16) { return __half2float(__ushort_as_half((unsigned short)bits16)); }
__device__ __forceinline__ uint32_t f2h(float x) { return (uint32_t)__half_as_ushort(__float2half_rn(x)); }
// §23.7
__device__ __forceinline__ uint32_t add16(uint32_t bits16, float v) { return f2h(min_(h2f(bits16) + v, 65504.0f)); }

__global__ __launch_bounds__(256) void star_kernel(const StarSet S, const float4* __restrict__ src, uint2* __restrict__ img, int W, int H) {
    __shared__ float4 tile[(TILE_H + 2) * TILE_P];
    __shared__ float4 corn[(TILE_H + 1) * CORN_P];
    const int bx = (int)blockIdx.x * TILE_W, by = (int)blockIdx.y * TILE_H;
    for (int i = (int)threadIdx.x; i < (TILE_H + 2) * TILE_P; i += 256) {
        const int ly = i / TILE_P, lx = i - ly * TILE_P;
        const int gx = bx + lx - 1, gy = by + ly - 1;
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
    if (!(k00.w != 0.0f && k10.w != 0.0f && k01.w != 0.0f && k11.w != 0.0f)) return;
    const float4 p = tile[(ty + 1) * TILE_P + tx + 1];
    F3 acc;
    const uint32_t n = star_pixel(S, f3(p.x, p.y, p.z), f3(k00.x, k00.y, k00.z), f3(k10.x, k10.y, k10.z), f3(k01.x, k01.y, k01.z), f3(k11.x, k11.y, k11.z), acc, nullptr);
    if (n == 0) return;
    const size_t o = (size_t)gy * (size_t)W + (size_t)gx;
    const uint2 q = img[o];
    const uint32_t r = add16(q.x & 0xffffu, acc.x * S.gain), g = add16(q.x >> 16, acc.y * S.gain), b = add16(q.y & 0xffffu, acc.z * S.gain);
    img[o] = make_uint2(r | (g << 16), b | (q.y & 0xffff0000u));
}

bool finite_f(float x) { return star_finite(x); }

}  // namespace

const char* stars_error(const bhray_star* stars, uint32_t n, const bhray_star_params* params) {
    if (params) {
        if (params->struct_size != sizeof(bhray_star_params)) return "bhray_star_params.struct_size is not sizeof(bhray_star_params)";
        if (!finite_f(params->gain) || !(params->gain > 0.0f)) return "gain must be finite and > 0";
        if (!finite_f(params->min_area) || !(params->min_area > 0.0f)) return "min_area must be finite and > 0";
        if (!(params->max_footprint > 0.0f && params->max_footprint <= 0.25f)) return "max_footprint must be in (0, 0.25]";
    }
    if (n > BHRAY_MAX_STARS) return "more than BHRAY_MAX_STARS stars";
    if (!stars) return nullptr;
    for (uint32_t i = 0; i < n; i++) {
        const bhray_star& s = stars[i];
        if (!finite_f(s.dir[0]) || !finite_f(s.dir[1]) || !finite_f(s.dir[2])) return "a star's dir is not finite";
        if (s.dir[0] == 0.0f && s.dir[1] == 0.0f && s.dir[2] == 0.0f) return "a star's dir is zero";
        for (int k = 0; k < 3; k++) if (!finite_f(s.flux[k]) || !(s.flux[k] >= 0.0f)) return "a star's flux is not finite and >= 0";
    }
    return nullptr;
}

void stars_build_index(const bhray_star* stars, uint32_t n, uint32_t& G, std::vector<float4>& sorted, std::vector<uint32_t>& prefix) {
    G = 1;
    (void)bhray_star_grid_size(n, &G);
    const size_t cells = 6u * (size_t)G * G;
    std::vector<uint32_t> cell(n);
    prefix.assign(cells + 1, 0u);
    for (uint32_t i = 0; i < n; i++) {
        cell[i] = star_cell_of(f3(stars[i].dir[0], stars[i].dir[1], stars[i].dir[2]), G);
        prefix[cell[i] + 1]++;
    }
    for (size_t k = 0; k < cells; k++) prefix[k + 1] += prefix[k];
    std::vector<uint32_t> at(prefix.begin(), prefix.end() - 1);
    sorted.assign(2u * (size_t)n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t i = 0; i < n; i++) {                                   // a counting sort in input order: (cell, original index)
        const size_t k = at[cell[i]]++;
        sorted[2 * k] = make_float4(stars[i].dir[0], stars[i].dir[1], stars[i].dir[2], 0.0f);
        sorted[2 * k + 1] = make_float4(stars[i].flux[0], stars[i].flux[1], stars[i].flux[2], 0.0f);
    }
}

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_stars(const StarSet& S, const float4* frame, uint2* sky, uint32_t frame_w, uint32_t frame_h, hipStream_t s) {
    if (frame_w == 0 || frame_h == 0) return hipSuccess;
    const unsigned gx = (frame_w + TILE_W - 1) / TILE_W, gy = (frame_h + TILE_H - 1) / TILE_H;
    if (gy > 65535u || frame_w > 32767u || !S.stars || !S.prefix || S.G < 1 || S.G > 1024 || (S.G & (S.G - 1)) != 0 || !frame || !sky) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(star_kernel, dim3(gx, gy), dim3(256), 0, s, S, frame, sky, (int)frame_w, (int)frame_h);
    return hipGetLastError();
}

}  // namespace bhray

using namespace bhray;

extern "C" void bhray_star_params_default(bhray_star_params* p) {
    if (!p) return;
    p->struct_size = (uint32_t)sizeof(bhray_star_params);
    p->gain = 1.0f; p->min_area = 1e-7f; p->max_footprint = 0.25f;
}

extern "C" int bhray_star_grid_size(uint32_t n, uint32_t* G) {
    if (!G || n > BHRAY_MAX_STARS) return BHRAY_E_INVALID;
    uint32_t g = 1;
    while (g < 1024u && 12ull * g * g < (uint64_t)n) g *= 2;
    *G = g;
    return BHRAY_OK;
}

extern "C" int bhray_star_cell(const float dir[3], uint32_t G, uint32_t* cell) {
    if (!dir || !cell || G < 1 || G > 1024 || (G & (G - 1)) != 0) return BHRAY_E_INVALID;
    if (!star_finite(dir[0]) || !star_finite(dir[1]) || !star_finite(dir[2]) || (dir[0] == 0.0f && dir[1] == 0.0f && dir[2] == 0.0f)) return BHRAY_E_INVALID;
    *cell = star_cell_of(f3(dir[0], dir[1], dir[2]), G);
    return BHRAY_OK;
}

// the host form over a frame: add (w x h x 4 floats, may be NULL) and per-pixel information (may be NULL)
int bhray::stars_resolve_host(const float* frame, uint32_t w, uint32_t h, bool wrap_x, const bhray_star* stars, uint32_t n, const bhray_star_params* params, float* add,
                              bhray_star_pixel_info* info) {
    if (!frame || !stars || n == 0 || w == 0 || h == 0 || w > 32767 || h > 32767 || (!add && !info)) return BHRAY_E_INVALID;
    if (stars_error(stars, n, params)) return BHRAY_E_INVALID;
    bhray_star_params P;
    bhray_star_params_default(&P);
    if (params) P = *params;
    uint32_t G;
    std::vector<float4> sorted; std::vector<uint32_t> prefix;
    stars_build_index(stars, n, G, sorted, prefix);
    StarSet S{sorted.data(), prefix.data(), G, P.gain, P.min_area, P.max_footprint * P.max_footprint};
    const float4* F = (const float4*)frame;
    const float4 out_px = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    auto px = [&](int x, int y) {
        if (wrap_x) x = x < 0 ? x + (int)w : x >= (int)w ? x - (int)w : x;   // §24: columns -1 and w are columns w - 1 and 0
        return (x >= 0 && y >= 0 && x < (int)w && y < (int)h) ? F[(size_t)y * w + (size_t)x] : out_px;
    };
    const size_t cw = (size_t)w + 1;
    std::vector<float4> corn(cw * ((size_t)h + 1));
    for (int y = 0; y <= (int)h; y++)
        for (int x = 0; x <= (int)w; x++) {
            F3 c;
            const bool ok = star_corner(px(x - 1, y - 1), px(x, y - 1), px(x - 1, y), px(x, y), c);
            corn[(size_t)y * cw + (size_t)x] = make_float4(c.x, c.y, c.z, ok ? 1.0f : 0.0f);
        }
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t o = (size_t)y * w + x;
            const float4 k00 = corn[(size_t)y * cw + x], k10 = corn[(size_t)y * cw + x + 1], k01 = corn[((size_t)y + 1) * cw + x], k11 = corn[((size_t)y + 1) * cw + x + 1];
            F3 acc = f3(0.0f, 0.0f, 0.0f);
            uint32_t got = 0;
            StarPixelInfo pi{};
            pi.state = 3;                                                // no footprint
            if (k00.w != 0.0f && k10.w != 0.0f && k01.w != 0.0f && k11.w != 0.0f) {
                const float4 p = F[o];
                got = star_pixel(S, f3(p.x, p.y, p.z), f3(k00.x, k00.y, k00.z), f3(k10.x, k10.y, k10.z), f3(k01.x, k01.y, k01.z), f3(k11.x, k11.y, k11.z), acc, &pi);
            }
            if (add) { float* a = add + 4 * o; a[0] = acc.x * S.gain; a[1] = acc.y * S.gain; a[2] = acc.z * S.gain; a[3] = (float)got; }
            if (info) {
                bhray_star_pixel_info& q = info[o];
                q.state = pi.state; q.faces = pi.faces; q.cells = pi.cells; q.tested = pi.tested; q.accepted = pi.accepted; q.reversed = pi.reversed; q.area = pi.area; q.pad = 0;
            }
        }
    return BHRAY_OK;
}

extern "C" int bhray_stars_resolve_host(const float* frame, uint32_t w, uint32_t h, const bhray_star* stars, uint32_t n, const bhray_star_params* params, float* add) {
    if (!add) return BHRAY_E_INVALID;
    return stars_resolve_host(frame, w, h, false, stars, n, params, add, nullptr);
}

extern "C" int bhray_diag_stars_pixel_info_host(const float* frame, uint32_t w, uint32_t h, const bhray_star* stars, uint32_t n, const bhray_star_params* params,
                                                bhray_star_pixel_info* info) {
    if (!info) return BHRAY_E_INVALID;
    return stars_resolve_host(frame, w, h, false, stars, n, params, nullptr, info);
}
