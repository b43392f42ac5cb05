// bhray_accum_passes.hip — the kernels of the still passes (bhray_accum_set_passes): what a still knows about every sample beside its colour.
//
//   accum_passes_add_kernel    the box form: one thread per pixel loops over the launch's K samples in sample order, forms each requested pass's (v, 1) through
//                              accum_pass_value and adds it to a register copy of that pass's sum; every plane is read once and stored once
//   accum_passes_form_kernel   the filtered form: one thread per ray writes one pass's sample image - (v, 1), all-NaN for a skipped sample - for
//                              accum_filter_add_kernel (bhray_accum_filter.hip, unchanged) to sum with the colour's stencil and weights
//
// Consecutive lanes on consecutive pixels (rays), every access one float4: a sample costs 48 bytes in (result, record) and 32 more with BHRAY_PASS_ESCAPE (the ray's
// direction half shares a 32-byte record with its origin), so the kernels are HBM-bound by construction.  No atomics: a pixel's sums have one writer.  Translation
// unit of its own, so that no pre-existing kernel's registers or schedule can move with it; compiled -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>

#include "bhray_accum_passes.h"

namespace bhray {
namespace {

__global__ __launch_bounds__(256) void accum_passes_add_kernel(const float4* __restrict__ results, const float4* __restrict__ records, const float4* __restrict__ rays,
                                                               const AccumPassPlanes planes, uint32_t passes, uint32_t npix, uint32_t k) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    float4 acc[ACCUM_PASS_COUNT];
#pragma unroll
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) acc[b] = (passes >> b) & 1u ? planes.plane[b][p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool escape = (passes & BHRAY_PASS_ESCAPE) != 0;
    for (uint32_t j = 0; j < k; j++) {
        const size_t i = (size_t)j * npix + p;
        const float4 R = results[i];
        const float4 qa = records[2 * i], qb = records[2 * i + 1];
        const float4 d = escape ? rays[2 * i + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) {
            if (!((passes >> b) & 1u)) continue;                  // uniform over the grid
            float4 v;
            if (accum_pass_value(1u << b, R, qa, qb, d, v)) { acc[b].x = acc[b].x + v.x; acc[b].y = acc[b].y + v.y; acc[b].z = acc[b].z + v.z; acc[b].w = acc[b].w + v.w; }
        }
    }
#pragma unroll
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) if ((passes >> b) & 1u) planes.plane[b][p] = acc[b];
}

__global__ __launch_bounds__(256) void accum_passes_form_kernel(const float4* __restrict__ results, const float4* __restrict__ records, const float4* __restrict__ rays,
                                                                uint32_t pass, float4* __restrict__ images, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 d = pass == BHRAY_PASS_ESCAPE ? rays[2 * i + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float nan = u2f(0x7fc00000u);
    float4 v = make_float4(nan, nan, nan, nan);
    (void)accum_pass_value(pass, results[i], records[2 * i], records[2 * i + 1], d, v);
    images[i] = v;
}

bool one_pass(uint32_t pass) { return pass != 0 && (pass & ~(uint32_t)BHRAY_PASS_ALL) == 0 && (pass & (pass - 1)) == 0; }

}  // namespace

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_accum_passes_add(const float4* results, const float4* records, const float4* rays, const AccumPassPlanes& planes, uint32_t passes, uint32_t npix,
                                   uint32_t k, hipStream_t s) {
    if (npix == 0 || k == 0 || passes == 0) return hipSuccess;
    if ((passes & ~(uint32_t)BHRAY_PASS_ALL) || !results || !records || ((passes & BHRAY_PASS_ESCAPE) && !rays) || (size_t)k * npix > ((size_t)1 << 26)) return hipErrorInvalidValue;
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) if (((passes >> b) & 1u) && !planes.plane[b]) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_passes_add_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, results, records, rays, planes, passes, npix, k);
    return hipGetLastError();
}

hipError_t launch_accum_passes_form(const float4* results, const float4* records, const float4* rays, uint32_t pass, float4* images, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!one_pass(pass) || !results || !records || !images || (pass == BHRAY_PASS_ESCAPE && !rays) || n > ((size_t)1 << 26)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_passes_form_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, results, records, rays, pass, images, n);
    return hipGetLastError();
}

}  // namespace bhray

// pure host arithmetic through accum_pass_value - no ctx, no device
extern "C" int bhray_accum_pass_values(const float* results, const bhray_ray_record* records, const bhray_ray* rays, uint32_t n, uint32_t pass, float* out) {
    if (!bhray::one_pass(pass) || (n != 0 && (!results || !records || !out || (pass == BHRAY_PASS_ESCAPE && !rays)))) return BHRAY_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const bhray_ray_record& q = records[i];
        const float4 R = make_float4(results[4 * (size_t)i], results[4 * (size_t)i + 1], results[4 * (size_t)i + 2], results[4 * (size_t)i + 3]);
        const float4 qa = make_float4(q.position[0], q.position[1], q.position[2], bhray::u2f(q.hit));
        const float4 qb = make_float4(bhray::u2f((uint32_t)q.triangle), bhray::u2f(q.iterations), q.closest, q.transmittance);
        const float4 d = rays ? make_float4(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2], 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        (void)bhray::accum_pass_value(pass, R, qa, qb, d, v);
        out[4 * (size_t)i] = v.x; out[4 * (size_t)i + 1] = v.y; out[4 * (size_t)i + 2] = v.z; out[4 * (size_t)i + 3] = v.w;
    }
    return BHRAY_OK;
}
