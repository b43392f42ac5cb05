// bhray_stillcam.hip — the kernels of the still cameras (bhray_accum_set_camera): the accumulation image's rays under a panorama, a fisheye or a thin lens.
//
//   still_gen_kernel        the bhray_ray records of K consecutive samples of every frame pixel, sample-major (accum_gen_kernel's layout)
//   still_gen_list_kernel   the records of the next sub-samples of the listed pixels (adapt_gen_kernel's layout)
//
// Both call still_record (bhray_stillcam.h), as the host form bhray_still_sample_rays_host does.  One thread per record, consecutive lanes on consecutive pixels, two
// float4 stores.  The accumulation launches them only while the camera in force is not "pinhole, no lens".  Translation unit of its own, so that no pre-existing
// kernel's registers or schedule can move with it.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

#include "bhray_stillcam.h"
#include "../../include/bhray_diag.h"

namespace bhray {
namespace {

// record i = j * npix + p: sample s0 + j through frame pixel p = y * frame_w + x, i.e. pixel (crop_x + x, crop_y + y) of the last level
__global__ __launch_bounds__(256) void still_gen_kernel(const StillGen g, float4* __restrict__ rays) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.a.k * g.a.npix) return;
    const uint32_t j = (uint32_t)(i / g.a.npix), p = (uint32_t)(i - (size_t)j * g.a.npix);
    const uint32_t y = p / g.a.frame_w, x = p - y * g.a.frame_w;
    float4 o, d;
    still_record(g, g.a.crop_x + x, g.a.crop_y + y, g.a.s0 + j, o, d);
    rays[2 * i] = o;
    rays[2 * i + 1] = d;
}

// record r = jj * n_active + i: sample issued[p] + j0 + jj through frame pixel p = list[i]
__global__ __launch_bounds__(256) void still_gen_list_kernel(const StillGen g, const uint32_t* __restrict__ list, uint32_t n_active, uint32_t j0,
                                                             const uint4* __restrict__ state, float4* __restrict__ rays) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.a.k * n_active) return;
    const uint32_t j = (uint32_t)(i / n_active), e = (uint32_t)(i - (size_t)j * n_active);
    const uint32_t p = list ? list[e] : e;
    const uint32_t s = state[p].z + j0 + j;
    const uint32_t y = p / g.a.frame_w, x = p - y * g.a.frame_w;
    float4 o, d;
    still_record(g, g.a.crop_x + x, g.a.crop_y + y, s, o, d);
    rays[2 * i] = o;
    rays[2 * i + 1] = d;
}

}  // namespace

const char* still_camera_error(const bhray_still_camera* cam) {
    if (!cam) return nullptr;                                     // NULL: the default
    if (cam->struct_size != sizeof(bhray_still_camera)) return "struct_size is not sizeof(bhray_still_camera)";
    if (cam->projection != BHRAY_STILL_PINHOLE && cam->projection != BHRAY_STILL_EQUIRECT && cam->projection != BHRAY_STILL_FISHEYE) return "unknown projection";
    if (cam->projection == BHRAY_STILL_FISHEYE && !(std::isfinite(cam->fisheye_fov) && cam->fisheye_fov > 0.0f && cam->fisheye_fov <= 6.28318548f))
        return "fisheye_fov must be finite and in (0, 2 pi]";
    if (!std::isfinite(cam->lens_radius) || cam->lens_radius < 0.0f) return "lens_radius must be finite and >= 0";
    if (cam->lens_radius > 0.0f) {
        if (cam->projection != BHRAY_STILL_PINHOLE) return "a lens needs the pinhole projection";
        if (!(std::isfinite(cam->focus_distance) && cam->focus_distance > 0.0f)) return "focus_distance must be finite and > 0 when lens_radius > 0";
    }
    return nullptr;
}

void still_gen_fill(StillGen& g, const bhray_config& cfg, const bhray_camera_uniform& cam, const bhray_still_camera& still) {
    memset(&g, 0, sizeof g);
    // derive_frame (bhray_api.hip): ray.wgsl:276-279
    const F3 fwd = ld3(cam.forward);
    const F3 right = normalize(cross(fwd, f3(0.0f, -1.0f, 0.0f)));
    const F3 up = normalize(cross(fwd, right));
    const float fov_factor = 1.0f / bh_tan(cam.fov / 2.0f);
    const F3 fwd_ff = fwd * fov_factor;
    const F3 fwd_n = normalize(fwd);
    memcpy(g.a.cam, cam.position, 12);
    g.a.right[0] = right.x; g.a.right[1] = right.y; g.a.right[2] = right.z;
    g.a.up[0] = up.x; g.a.up[1] = up.y; g.a.up[2] = up.z;
    g.a.fwd_ff[0] = fwd_ff.x; g.a.fwd_ff[1] = fwd_ff.y; g.a.fwd_ff[2] = fwd_ff.z;
    g.fwd_n[0] = fwd_n.x; g.fwd_n[1] = fwd_n.y; g.fwd_n[2] = fwd_n.z;
    // accum_gen_args: the last level's constants
    const int lw = (int)cfg.level_w[cfg.levels - 1], lh = (int)cfg.level_h[cfg.levels - 1];
    const int sm = (lw - 1) < (lh - 1) ? (lw - 1) : (lh - 1);
    g.a.half_w = (float)(lw - 1) * 0.5f; g.a.half_h = (float)(lh - 1) * 0.5f;
    g.a.increment = 1.0f / (float)sm;
    g.a.crop_x = cfg.crop_x; g.a.crop_y = cfg.crop_y; g.a.frame_w = cfg.frame_w;
    g.a.npix = cfg.frame_w * cfg.frame_h;
    g.lon_scale = 6.28318548f / (float)lw;
    g.lat_scale = 3.14159274f / (float)lh;
    g.radius = (float)sm * 0.5f;
    g.projection = still.projection;
    g.level_w = (uint32_t)lw;
    if (still.projection == BHRAY_STILL_FISHEYE) g.half_fov = still.fisheye_fov * 0.5f;
    if (still.projection == BHRAY_STILL_PINHOLE && still.lens_radius > 0.0f) { g.lens_radius = still.lens_radius; g.focus = still.focus_distance; }
}

// (launchers report the error of THEIR launch: HIP's last-error state is sticky, so it is cleared first - as bhray_kernels.hip's)
hipError_t launch_still_gen(const StillGen& g, float4* rays, hipStream_t s) {
    const size_t n = (size_t)g.a.k * g.a.npix;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.a.frame_w == 0 || !rays) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(still_gen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, rays);
    return hipGetLastError();
}

hipError_t launch_still_gen_list(const StillGen& g, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state, float4* rays, hipStream_t s) {
    const size_t n = (size_t)g.a.k * n_active;
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 26) || g.a.frame_w == 0 || n_active > g.a.npix || !state || !rays) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(still_gen_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, list, n_active, j0, state, rays);
    return hipGetLastError();
}

}  // namespace bhray

extern "C" void bhray_still_camera_default(bhray_still_camera* cam) {
    if (!cam) return;
    memset(cam, 0, sizeof *cam);
    cam->struct_size = (uint32_t)sizeof(bhray_still_camera);
    cam->projection = BHRAY_STILL_PINHOLE;
    cam->fisheye_fov = 3.14159274f;
    cam->focus_distance = 1.0f;
}

// bhray_diag.h: pure host arithmetic through still_record - no ctx, no device
extern "C" int bhray_still_sample_rays_host(const bhray_config* cfg, const void* camera_uniform_32, const bhray_still_camera* camera, uint32_t s, bhray_ray* out) {
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
    for (uint32_t y = 0; y < cfg->frame_h; y++)
        for (uint32_t x = 0; x < cfg->frame_w; x++) {
            float4 o, d;
            bhray::still_record(g, cfg->crop_x + x, cfg->crop_y + y, s, o, d);
            bhray_ray& r = out[(size_t)y * cfg->frame_w + x];
            r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.pad0 = 0.0f;
            r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.pad1 = 0.0f;
        }
    return BHRAY_OK;
}
