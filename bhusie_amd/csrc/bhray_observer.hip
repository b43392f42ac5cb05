// bhray_observer.hip — the kernels of the moving observer of stills (bhray_accum_set_observer): aberration before the trace, beaming behind it.
//
//   observer_gen_kernel         the bhray_ray records of K consecutive samples of every frame pixel, sample-major (still_gen_kernel's layout), boosted
//   observer_gen_list_kernel    the records of the next sub-samples of the listed pixels (still_gen_list_kernel's layout), boosted
//   observer_beam_kernel        between a launch's trace (and its star stage) and its add: every result of the launch resolved and scaled by its record's D^4, in place
//   observer_beam_list_kernel   the same over an adaptive round's records
//
// All four call observer_record (bhray_observer.h), as the host forms bhray_observer_sample_rays_host and bhray_observer_boost_rays do.  One thread per record,
// consecutive lanes on consecutive pixels; the generators store two float4, the beam kernels load and store one and read the sky texture only where w == 0.  No LDS,
// no atomics.  The accumulation launches them only while an observer with a velocity other than zero is in force.  Translation unit of its own, so that no pre-existing
// kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

#include "bhray_observer.h"
#include "bhray_tex.h"
#include "../../include/bhray_diag.h"

namespace bhray {
namespace {

// record i = j * npix + p: sample s0 + j through frame pixel p = y * frame_w + x, i.e. pixel (crop_x + x, crop_y + y) of the last level
__global__ __launch_bounds__(256) void observer_gen_kernel(const StillGen g, const ObserverDev o, float4* __restrict__ rays) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.a.k * g.a.npix) return;
    const uint32_t j = (uint32_t)(i / g.a.npix), p = (uint32_t)(i - (size_t)j * g.a.npix);
    const uint32_t y = p / g.a.frame_w, x = p - y * g.a.frame_w;
    float4 org, d;
    float beam;
    observer_record(g, o, g.a.crop_x + x, g.a.crop_y + y, g.a.s0 + j, org, d, beam);
    rays[2 * i] = org;
    rays[2 * i + 1] = d;
}

// record r = jj * n_active + i: sample issued[p] + j0 + jj through frame pixel p = list[i]
__global__ __launch_bounds__(256) void observer_gen_list_kernel(const StillGen g, const ObserverDev o, const uint32_t* __restrict__ list, uint32_t n_active, uint32_t j0,
                                                                const uint4* __restrict__ state, float4* __restrict__ rays) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.a.k * n_active) return;
    const uint32_t j = (uint32_t)(i / n_active), e = (uint32_t)(i - (size_t)j * n_active);
    const uint32_t p = list ? list[e] : e;
    const uint32_t s = state[p].z + j0 + j;
    const uint32_t y = p / g.a.frame_w, x = p - y * g.a.frame_w;
    float4 org, d;
    float beam;
    observer_record(g, o, g.a.crop_x + x, g.a.crop_y + y, s, org, d, beam);
    rays[2 * i] = org;
    rays[2 * i + 1] = d;
}

// the beam of record (lx, ly, s) onto img[i]: resolved where it is a direction pixel, colour times B, alpha kept; an all-zero rest-frame direction leaves it alone
__device__ __forceinline__ void beam_one(const StillGen& g, const ObserverDev& o, const TexDev& sky, uint32_t lx, uint32_t ly, uint32_t s, float4* __restrict__ img, size_t i) {
    float4 org, d;
    float B;
    still_record(g, lx, ly, s, org, d);
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return;
    observer_boost(o, d.x, d.y, d.z, B);
    float4 v = resolve(sky, img[i]);
    v.x = v.x * B; v.y = v.y * B; v.z = v.z * B;
    img[i] = v;
}

__global__ __launch_bounds__(256) void observer_beam_kernel(const StillGen g, const ObserverDev o, const TexDev sky, float4* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.a.k * g.a.npix) return;
    const uint32_t j = (uint32_t)(i / g.a.npix), p = (uint32_t)(i - (size_t)j * g.a.npix);
    const uint32_t y = p / g.a.frame_w, x = p - y * g.a.frame_w;
    beam_one(g, o, sky, g.a.crop_x + x, g.a.crop_y + y, g.a.s0 + j, img, i);
}

__global__ __launch_bounds__(256) void observer_beam_list_kernel(const StillGen g, const ObserverDev o, const TexDev sky, const uint32_t* __restrict__ list, uint32_t n_active,
                                                                 uint32_t j0, const uint4* __restrict__ state, float4* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.a.k * n_active) return;
    const uint32_t j = (uint32_t)(i / n_active), e = (uint32_t)(i - (size_t)j * n_active);
    const uint32_t p = list ? list[e] : e;
    const uint32_t s = state[p].z + j0 + j;
    const uint32_t y = p / g.a.frame_w, x = p - y * g.a.frame_w;
    beam_one(g, o, sky, g.a.crop_x + x, g.a.crop_y + y, s, img, i);
}

// bb = (bx*bx + by*by) + bz*bz, the header's order
float speed2(const float* b) { return (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]; }

void store_ray(bhray_ray& r, const float4& o, const float4& d) {
    r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.pad0 = 0.0f;
    r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.pad1 = 0.0f;
}

}  // namespace

const char* observer_error(const bhray_observer* obs) {
    if (!obs) return nullptr;                                     // NULL: at rest
    if (obs->struct_size != sizeof(bhray_observer)) return "struct_size is not sizeof(bhray_observer)";
    if (!std::isfinite(obs->velocity[0]) || !std::isfinite(obs->velocity[1]) || !std::isfinite(obs->velocity[2])) return "velocity must be finite";
    if (speed2(obs->velocity) > BHRAY_OBSERVER_MAX_SPEED2) return "the speed exceeds 0.99 c (BHRAY_OBSERVER_MAX_SPEED2)";
    if (obs->beaming > 1u) return "beaming must be 0 or 1";
    return nullptr;
}

void observer_fill(ObserverDev& o, const bhray_observer& obs) {
    memcpy(o.b, obs.velocity, 12);
    const float bb = speed2(o.b);
    o.ig = sqrtf(1.0f - bb);
    const float g = 1.0f / o.ig;
    o.k = g / (g + 1.0f);
}

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_observer_gen(const StillGen& g, const ObserverDev& o, float4* rays, hipStream_t s) {
    const size_t n = (size_t)g.a.k * g.a.npix;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.a.frame_w == 0 || !rays) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(observer_gen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, o, rays);
    return hipGetLastError();
}

hipError_t launch_observer_gen_list(const StillGen& g, const ObserverDev& o, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state, float4* rays, hipStream_t s) {
    const size_t n = (size_t)g.a.k * n_active;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.a.frame_w == 0 || n_active > g.a.npix || !state || !rays) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(observer_gen_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, o, list, n_active, j0, state, rays);
    return hipGetLastError();
}

hipError_t launch_observer_beam(const StillGen& g, const ObserverDev& o, const TexDev& sky, float4* img, hipStream_t s) {
    const size_t n = (size_t)g.a.k * g.a.npix;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.a.frame_w == 0 || !img || !sky.rgba || sky.w < 1 || sky.h < 1) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(observer_beam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, o, sky, img);
    return hipGetLastError();
}

hipError_t launch_observer_beam_list(const StillGen& g, const ObserverDev& o, const TexDev& sky, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state,
                                     float4* img, hipStream_t s) {
    const size_t n = (size_t)g.a.k * n_active;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.a.frame_w == 0 || n_active > g.a.npix || !state || !img || !sky.rgba || sky.w < 1 || sky.h < 1) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(observer_beam_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, o, sky, list, n_active, j0, state, img);
    return hipGetLastError();
}

}  // namespace bhray

extern "C" void bhray_observer_default(bhray_observer* obs) {
    if (!obs) return;
    memset(obs, 0, sizeof *obs);
    obs->struct_size = (uint32_t)sizeof(bhray_observer);
    obs->beaming = 1u;
}

// bhray.h: host arithmetic through observer_boost - no ctx, no device
extern "C" int bhray_observer_boost_rays(const bhray_observer* obs, const bhray_ray* in, uint32_t n, bhray_ray* out, float* out_beam) {
    if (n != 0 && (!in || !out)) return BHRAY_E_INVALID;
    if (bhray::observer_error(obs)) return BHRAY_E_INVALID;
    const bool rest = !obs || bhray::observer_at_rest(*obs);
    bhray::ObserverDev o{};
    if (!rest) bhray::observer_fill(o, *obs);
    for (uint32_t i = 0; i < n; i++) {
        bhray_ray r = in[i];
        float beam = 1.0f;
        if (!rest && !(r.direction[0] == 0.0f && r.direction[1] == 0.0f && r.direction[2] == 0.0f))
            bhray::observer_boost(o, r.direction[0], r.direction[1], r.direction[2], beam);
        out[i] = r;
        if (out_beam) out_beam[i] = beam;
    }
    return BHRAY_OK;
}

// bhray_diag.h: bhray_still_sample_rays_host through observer_record
extern "C" int bhray_observer_sample_rays_host(const bhray_config* cfg, const void* camera_uniform_32, const bhray_still_camera* camera, const bhray_observer* observer, uint32_t s,
                                               bhray_ray* out, float* out_beam) {
    if (bhray::observer_error(observer)) return BHRAY_E_INVALID;
    if (!observer || bhray::observer_at_rest(*observer)) {        // no observer: the still camera's records, beam 1
        const int rc = bhray_still_sample_rays_host(cfg, camera_uniform_32, camera, s, out);
        if (rc == BHRAY_OK && out_beam)
            for (size_t i = 0, n = (size_t)cfg->frame_w * cfg->frame_h; i < n; i++) out_beam[i] = 1.0f;
        return rc;
    }
    if (!cfg || !camera_uniform_32 || !out || s >= BHRAY_ACCUM_MAX_SAMPLES) return BHRAY_E_INVALID;
    if (cfg->struct_size != sizeof(bhray_config) || cfg->levels < 1 || cfg->levels > BHRAY_MAX_LEVELS) return BHRAY_E_INVALID;
    const uint32_t lw = cfg->level_w[cfg->levels - 1], lh = cfg->level_h[cfg->levels - 1];
    if (lw < 2 || lh < 2 || cfg->frame_w == 0 || cfg->frame_h == 0 || cfg->frame_w > lw || cfg->frame_h > lh || cfg->crop_x > lw - cfg->frame_w || cfg->crop_y > lh - cfg->frame_h)
        return BHRAY_E_INVALID;
    if (bhray::still_camera_error(camera)) return BHRAY_E_INVALID;
    bhray_still_camera still;
    if (camera) still = *camera; else bhray_still_camera_default(&still);
    bhray_camera_uniform cam;
    memcpy(&cam, camera_uniform_32, sizeof cam);
    bhray::StillGen g;
    bhray::still_gen_fill(g, *cfg, cam, still);
    bhray::ObserverDev o;
    bhray::observer_fill(o, *observer);
    for (uint32_t y = 0; y < cfg->frame_h; y++)
        for (uint32_t x = 0; x < cfg->frame_w; x++) {
            float4 org, d;
            float beam;
            bhray::observer_record(g, o, cfg->crop_x + x, cfg->crop_y + y, s, org, d, beam);
            const size_t i = (size_t)y * cfg->frame_w + x;
            bhray::store_ray(out[i], org, d);
            if (out_beam) out_beam[i] = beam;
        }
    return BHRAY_OK;
}
