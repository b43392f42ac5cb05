// bhray_accum_filter.hip — the kernel of the still pixel filters (bhray_accum_set_filter): tent and cubic reconstruction of the accumulation image.
//
//   accum_filter_add_kernel   accum_add_kernel's place under a filter other than the box: per sample a 5 x 5 separable stencil over that sample's resolved results
//
// Sample s has one sub-pixel offset for all pixels, so a wider filter is no scatter: pixel p gathers sample s of the 25 pixels around it with ten weights that are the
// same for every pixel.  A block is four waves on a 32 x 8 pixel tile.  For each of the launch's K samples, in order, it loads the tile plus a halo of 2 (36 x 12
// texels) from the sample-major result buffer, resolves each texel ONCE at load (alpha == 0 -> sky^4; outside the frame or not finite -> zeros with weight 0: a
// select, never 0 * NaN) and stores it as a float4 in LDS (6912 bytes); lanes 0 .. 9 evaluate the sample's ten weights (accum_filter_tap, the function
// bhray_accum_filter_weights calls on the host) into LDS beside it.  After the barrier every thread forms the five row sums and their column sum in registers, in the
// contract's order, and adds it to a register copy of sum[p], which is stored once per launch.  No atomics: a pixel's sum has one writer.  A 32-lane half of a wave
// is 32 consecutive pixels of one row, so its float4 LDS reads fall on consecutive 16-byte slots and every 16-lane group of the read covers 16 distinct slots of the
// 256-byte bank row: conflict-free; the weights are broadcast reads.  The halo texels are the interior texels of the neighbouring blocks, which run at about the same
// time: L2 hits.  Translation unit of its own, so that no pre-existing kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

#include "bhray_accum_filter.h"
#include "bhray_tex.h"

namespace bhray {
namespace {

constexpr int TILE_W = 32, TILE_H = 8, HALO = 2;                  // tile of a block and the filter's reach
constexpr int TILE_P = TILE_W + 2 * HALO, TILE_R = TILE_H + 2 * HALO;   // pitch and rows of its LDS copy
static_assert(TILE_W * TILE_H == 256 && TILE_W == 32, "a 32-lane half of a wave is one row of the tile");

__global__ __launch_bounds__(256) void accum_filter_add_kernel(const TexDev sky, const AccumFilter f, const float4* __restrict__ results, float4* __restrict__ sum,
                                                               int W, int H, uint32_t s0, uint32_t k) {
    __shared__ float4 tile[TILE_R * TILE_P];
    __shared__ float wts[16];
    const int tid = (int)threadIdx.x;
    const int bx = (int)blockIdx.x * TILE_W, by = (int)blockIdx.y * TILE_H;
    const int tx = tid & (TILE_W - 1), ty = tid >> 5;
    const int gx = bx + tx, gy = by + ty;
    const bool inside = gx < W && gy < H;                         // (a thread outside the frame still loads and meets the barriers)
    const size_t npix = (size_t)W * (size_t)H;
    const size_t p = (size_t)gy * (size_t)W + (size_t)gx;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside) acc = sum[p];
    for (uint32_t j = 0; j < k; j++) {
        const float4* __restrict__ res = results + (size_t)j * npix;
        for (int i = tid; i < TILE_R * TILE_P; i += 256) {
            const int ly = i / TILE_P, lx = i - ly * TILE_P;
            const int x = bx + lx - HALO, y = by + ly - HALO;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);       // outside the frame, or a sample that is skipped: no colour, no weight
            if (x >= 0 && x < W && y >= 0 && y < H) {
                const float4 r = resolve(sky, res[(size_t)y * (size_t)W + (size_t)x]);
                if (finite_(r.x) && finite_(r.y) && finite_(r.z)) v = make_float4(r.x, r.y, r.z, 1.0f);
            }
            tile[i] = v;
        }
        if (tid < 10) wts[tid] = accum_filter_tap(f, s0 + j, (uint32_t)tid);
        __syncthreads();
        float wx[5], wy[5];
#pragma unroll
        for (int i = 0; i < 5; i++) { wx[i] = wts[i]; wy[i] = wts[5 + i]; }
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int jj = 0; jj < 5; jj++) {
            float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int ii = 0; ii < 5; ii++) {
                const float4 v = tile[(ty + jj) * TILE_P + tx + ii];
                row.x = row.x + wx[ii] * v.x; row.y = row.y + wx[ii] * v.y; row.z = row.z + wx[ii] * v.z; row.w = row.w + wx[ii] * v.w;
            }
            c.x = c.x + wy[jj] * row.x; c.y = c.y + wy[jj] * row.y; c.z = c.z + wy[jj] * row.z; c.w = c.w + wy[jj] * row.w;
        }
        acc.x = acc.x + c.x; acc.y = acc.y + c.y; acc.z = acc.z + c.z; acc.w = acc.w + c.w;
        __syncthreads();                                          // the next sample's load rewrites the tile and the weights
    }
    if (inside) sum[p] = acc;
}

bool in_range(float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; }

}  // namespace

const char* still_filter_error(const bhray_still_filter* filter) {
    if (!filter) return nullptr;                                  // NULL: the default
    if (filter->struct_size != sizeof(bhray_still_filter)) return "struct_size is not sizeof(bhray_still_filter)";
    if (filter->kind == BHRAY_FILTER_BOX) return nullptr;
    if (filter->kind == BHRAY_FILTER_TENT) return in_range(filter->radius, 0.5f, 2.5f) ? nullptr : "a tent's radius must be finite and in [0.5, 2.5]";
    if (filter->kind != BHRAY_FILTER_CUBIC) return "unknown kind";
    if (!in_range(filter->radius, 1.0f, 2.5f)) return "a cubic's radius must be finite and in [1, 2.5]";
    if (!in_range(filter->b, 0.0f, 1.0f) || !in_range(filter->c, 0.0f, 1.0f)) return "a cubic's b and c must be finite and in [0, 1]";
    return nullptr;
}

void accum_filter_fill(AccumFilter& f, const bhray_still_filter& filter) {
    memset(&f, 0, sizeof f);
    f.kind = filter.kind;
    if (filter.kind == BHRAY_FILTER_TENT) f.radius = filter.radius;
    if (filter.kind == BHRAY_FILTER_CUBIC) {
        const double B = (double)filter.b, C = (double)filter.c;
        f.inv = 2.0f / filter.radius;
        f.p3 = (float)((12.0 - 9.0 * B - 6.0 * C) / 6.0); f.p2 = (float)((-18.0 + 12.0 * B + 6.0 * C) / 6.0); f.p0 = (float)((6.0 - 2.0 * B) / 6.0);
        f.q3 = (float)((-B - 6.0 * C) / 6.0); f.q2 = (float)((6.0 * B + 30.0 * C) / 6.0); f.q1 = (float)((-12.0 * B - 48.0 * C) / 6.0); f.q0 = (float)((8.0 * B + 24.0 * C) / 6.0);
    }
}

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_accum_filter_add(const TexDev& sky, const AccumFilter& f, const float4* results, float4* sum, uint32_t frame_w, uint32_t frame_h, uint32_t s0, uint32_t k,
                                   hipStream_t s) {
    if (frame_w == 0 || frame_h == 0 || k == 0) return hipSuccess;
    const unsigned gx = (frame_w + TILE_W - 1) / TILE_W, gy = (frame_h + TILE_H - 1) / TILE_H;
    if (gy > 65535u || frame_w > (1u << 30) || frame_h > (1u << 30) || !results || !sum || (f.kind != BHRAY_FILTER_TENT && f.kind != BHRAY_FILTER_CUBIC)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_filter_add_kernel, dim3(gx, gy), dim3(256), 0, s, sky, f, results, sum, (int)frame_w, (int)frame_h, s0, k);
    return hipGetLastError();
}

}  // namespace bhray

extern "C" void bhray_still_filter_default(bhray_still_filter* filter) {
    if (!filter) return;
    memset(filter, 0, sizeof *filter);
    filter->struct_size = (uint32_t)sizeof(bhray_still_filter);
    filter->kind = BHRAY_FILTER_BOX;
    filter->radius = 2.0f;
    filter->b = filter->c = 1.0f / 3.0f;
}

// pure host arithmetic through accum_filter_tap - no ctx, no device
extern "C" int bhray_accum_filter_weights(const bhray_still_filter* filter, uint32_t s, float wx[5], float wy[5]) {
    if (!filter || !wx || !wy || bhray::still_filter_error(filter)) return BHRAY_E_INVALID;
    bhray::AccumFilter f;
    bhray::accum_filter_fill(f, *filter);
    for (uint32_t n = 0; n < 5; n++) { wx[n] = bhray::accum_filter_tap(f, s, n); wy[n] = bhray::accum_filter_tap(f, s, 5 + n); }
    return BHRAY_OK;
}
