// bhray_adapt.hip — the kernels of adaptive stills (bhray_accum_add_adaptive): each pixel is sampled until the error of its mean is under a bound.
//
//   adapt_select_kernel   the per-pixel test, and the indices of the pixels that fail it and may take more compacted into a list
//   adapt_gen_kernel      the bhray_ray records of the next sub-samples of the listed pixels, sample-major (what the ray-list trace kernels read)
//   adapt_add_kernel      resolve and add a listed pixel's results to its sum and to the two moments of its compressed luminance, in sample order
//   adapt_counts_kernel   the per-pixel sample counts out of the state records
//
// One thread per pixel / record / list entry, every state access one 16-byte word.  No atomics on the image: a pixel occurs once in a list, so its words have one
// writer, and the order of its additions is the sample order whatever the list's order and the cut of a round into launches.  Translation unit of its own, so that no
// pre-existing kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>

#include "bhray_adapt.h"
#include "bhray_tex.h"

namespace bhray {
namespace {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the test of include/bhray.h, one rounded operation per line; a comparison with a NaN is false
__device__ __forceinline__ bool converged(float n, float s1, float s2, float tolerance, float dark) {
    const float m = s1 / n;
    const float q = s2 / n;
    float v = q - m * m;
    v = v < 0.0f ? 0.0f : v;
    const float e = tolerance * (m + dark);
    return v <= (e * e) * n;
}

// 256 threads = 4 waves: ballot and popcount per wave, the four counts combined in LDS to one device-scope atomicAdd per block (block_append's shape, bhray_kernels.hip)
__global__ __launch_bounds__(256) void adapt_select_kernel(const float4* __restrict__ sum, const uint4* __restrict__ state, uint32_t npix, uint32_t max_samples,
                                                           float tolerance, float dark, uint32_t* __restrict__ list, uint32_t* __restrict__ ctl) {
    __shared__ uint32_t base[4], top[4];
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool want = false;
    uint32_t issued = 0;
    if (p < npix) {
        const uint4 st = state[p];
        issued = st.z;
        want = issued < max_samples && !converged(sum[p].w, u2f(st.x), u2f(st.y), tolerance, dark);
    }
    const unsigned long long m = __ballot(want);
    uint32_t hi = want ? issued : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)hi, off); hi = o > hi ? o : hi; }
    if (lane == 0) { base[wave] = (uint32_t)__popcll(m); top[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c0 = base[0], c1 = base[1], c2 = base[2], c3 = base[3], total = (c0 + c1) + (c2 + c3);
        uint32_t b = 0;
        if (total) {
            b = atomicAdd(&ctl[0], total);
            uint32_t t = top[0];
            t = top[1] > t ? top[1] : t; t = top[2] > t ? top[2] : t; t = top[3] > t ? top[3] : t;
            atomicMax(&ctl[1], t);
        }
        base[0] = b; base[1] = b + c0; base[2] = b + c0 + c1; base[3] = b + c0 + c1 + c2;
    }
    __syncthreads();
    if (want) list[base[wave] + lanes_below(m)] = p;          // at most npix pixels want: every slot lies in list[0 .. npix)
}

// record r = jj * n_active + i: sample issued[p] + j0 + jj through frame pixel p = list[i] = y * frame_w + x, i.e. pixel (crop_x + x, crop_y + y) of the last level
__global__ __launch_bounds__(256) void adapt_gen_kernel(const AccumGen g, const uint32_t* __restrict__ list, uint32_t n_active, uint32_t j0,
                                                        const uint4* __restrict__ state, float4* __restrict__ rays) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.k * n_active) return;
    const uint32_t j = (uint32_t)(i / n_active), e = (uint32_t)(i - (size_t)j * n_active);
    const uint32_t p = list ? list[e] : e;
    const uint32_t s = state[p].z + j0 + j;
    const uint32_t y = p / g.frame_w, x = p - y * g.frame_w;
    float dx, dy;
    accum_offset(s, dx, dy);
    const float px = (float)(g.crop_x + x) + dx, py = (float)(g.crop_y + y) + dy;
    // create_ray, ray.wgsl:269-285, as the trace kernels' refill forms it (right / up / fwd_ff and the level's constants from the host): accum_gen_kernel's operations
    const float posx = (2.0f * (px - g.half_w)) * g.increment;
    const float posy = (2.0f * (py - g.half_h)) * g.increment;
    const F3 rdir = normalize((ld3(g.right) * posx + ld3(g.up) * posy) + ld3(g.fwd_ff));
    rays[2 * i] = make_float4(g.cam[0], g.cam[1], g.cam[2], 0.0f);
    rays[2 * i + 1] = make_float4(rdir.x, rdir.y, rdir.z, 0.0f);
}

__global__ __launch_bounds__(256) void adapt_add_kernel(const TexDev sky, const float4* __restrict__ results, const uint32_t* __restrict__ list, uint32_t n_active,
                                                        uint32_t k, uint32_t advance, float4* __restrict__ sum, uint4* __restrict__ state) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_active) return;
    const uint32_t p = list ? list[i] : i;
    float4 acc = sum[p];
    const uint4 st = state[p];
    float s1 = u2f(st.x), s2 = u2f(st.y);
    for (uint32_t j = 0; j < k; j++) {
        const float4 r = resolve(sky, results[(size_t)j * n_active + i]);
        if (finite_(r.x) && finite_(r.y) && finite_(r.z)) {
            acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += 1.0f;
            float Y = (0.2126f * r.x + 0.7152f * r.y) + 0.0722f * r.z;
            Y = Y < 0.0f ? 0.0f : Y;
            const float t = Y >= 0x1p100f ? 1.0f : Y / (1.0f + Y);
            s1 += t;
            s2 += t * t;
        }
    }
    sum[p] = acc;
    state[p] = make_uint4(f2u(s1), f2u(s2), st.z + advance, 0u);
}

__global__ __launch_bounds__(256) void adapt_counts_kernel(const uint4* __restrict__ state, uint32_t* __restrict__ counts, uint32_t npix) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p < npix) counts[p] = state[p].z;
}

}  // namespace

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_adapt_select(const float4* sum, const uint4* state, uint32_t npix, uint32_t max_samples, float tolerance, float dark, uint32_t* list, uint32_t* ctl,
                               hipStream_t s) {
    if (npix == 0) return hipSuccess;
    if (!sum || !state || !list || !ctl) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(adapt_select_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, sum, state, npix, max_samples, tolerance, dark, list, ctl);
    return hipGetLastError();
}

hipError_t launch_adapt_gen(const AccumGen& g, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state, float4* rays, hipStream_t s) {
    const size_t n = (size_t)g.k * n_active;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.frame_w == 0 || n_active > g.npix || !state || !rays) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(adapt_gen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, list, n_active, j0, state, rays);
    return hipGetLastError();
}

hipError_t launch_adapt_add(const TexDev& sky, const float4* results, const uint32_t* list, uint32_t n_active, uint32_t k, uint32_t advance, float4* sum, uint4* state,
                            hipStream_t s) {
    if (n_active == 0 || k == 0) return hipSuccess;
    if (!results || !sum || !state) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(adapt_add_kernel, dim3((n_active + 255) / 256), dim3(256), 0, s, sky, results, list, n_active, k, advance, sum, state);
    return hipGetLastError();
}

hipError_t launch_adapt_counts(const uint4* state, uint32_t* counts, uint32_t npix, hipStream_t s) {
    if (npix == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(adapt_counts_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, state, counts, npix);
    return hipGetLastError();
}

}  // namespace bhray
