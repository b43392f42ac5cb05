// bhray_stillcam.h — still cameras (bhray_accum_set_camera): the accumulation image's camera model, evaluated on the device.  What the engine
// (bhray_api.hip) passes to the kernels of bhray_stillcam.hip, and the one function - still_record - that forms a sample's ray record on the device and on the host.
#pragma once
#include "bhray_accum.h"

namespace bhray {

// AccumGen (create_ray's constants on the ladder's last level) and what the other projections and the lens read: every member formed on the host, one rounded
// binary32 operation each
struct StillGen {
    AccumGen a;
    float fwd_n[3];            // normalize(forward)
    float lon_scale;           // 6.28318548f / float(lw)
    float lat_scale;           // 3.14159274f / float(lh)
    float radius;              // float(min(lw - 1, lh - 1)) * 0.5f: the fisheye's image circle
    float half_fov;            // fisheye_fov * 0.5f
    float lens_radius, focus;  // the thin lens (PINHOLE, lens_radius > 0)
    uint32_t projection;       // BHRAY_STILL_*
    uint32_t level_w;          // lw: the lens hash is of the level pixel index ly * lw + lx
};

BH_HD uint32_t still_hash(uint32_t v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

// The record of sample s through pixel (lx, ly) of the last level: include/bhray.h's contract, operation by operation (the TU is compiled -ffp-contract=off).
BH_HD void still_record(const StillGen& g, uint32_t lx, uint32_t ly, uint32_t s, float4& origin, float4& direction) {
    float dx, dy;
    accum_offset(s, dx, dy);
    const float px = (float)lx + dx, py = (float)ly + dy;
    const F3 right = ld3(g.a.right), up = ld3(g.a.up);
    F3 org = ld3(g.a.cam), dir;
    if (g.projection == BHRAY_STILL_EQUIRECT) {
        const float lon = (px - g.a.half_w) * g.lon_scale;
        const float lat = (py - g.a.half_h) * g.lat_scale;
        const float cl = bh_sincos<1>(lon), sl = bh_sincos<0>(lon);
        const float cp = bh_sincos<1>(lat), sp = bh_sincos<0>(lat);
        dir = normalize((ld3(g.fwd_n) * (cp * cl) + right * (cp * sl)) + up * sp);
    } else if (g.projection == BHRAY_STILL_FISHEYE) {
        const float X = (px - g.a.half_w) / g.radius;
        const float Y = (py - g.a.half_h) / g.radius;
        const float r = sqrtf(X * X + Y * Y);
        const float theta = r * g.half_fov;
        const float safe = r > 0.0f ? r : 1.0f;                   // r == 0: the centre, sin(theta) = 0 - the image direction does not matter
        const float cphi = X / safe, sphi = Y / safe;
        const float st = bh_sincos<0>(theta), ct = bh_sincos<1>(theta);
        dir = normalize((ld3(g.fwd_n) * ct + right * (st * cphi)) + up * (st * sphi));
        if (!(r <= 1.0f)) dir = f3(0.0f, 0.0f, 0.0f);             // outside the image circle: unusable, answered (0, 0, 0, -1) by the ray-list kernels
    } else {
        // create_ray, ray.wgsl:269-285: accum_gen_kernel's operations
        const float posx = (2.0f * (px - g.a.half_w)) * g.a.increment;
        const float posy = (2.0f * (py - g.a.half_h)) * g.a.increment;
        dir = normalize((right * posx + up * posy) + ld3(g.a.fwd_ff));
        if (g.lens_radius > 0.0f) {
            // the lens point: two Kronecker sequences (golden ratio, sqrt 2) rotated by a hash of the level pixel, onto the disk by the polar map
            const uint32_t q = ly * g.level_w + lx;
            const uint32_t a = still_hash(q) + s * 0x9E3779B9u;
            const uint32_t b = still_hash(q ^ 0x9E3779B9u) + s * 0x6A09E667u;
            const float ru = (float)(a >> 8) * 0x1p-24f;
            const float rv = (float)(b >> 8) * 0x1p-24f;
            const float rr = sqrtf(ru);
            const float ang = rv * 6.28318548f;
            const float ex = (rr * bh_sincos<1>(ang)) * g.lens_radius;
            const float ey = (rr * bh_sincos<0>(ang)) * g.lens_radius;
            const F3 off = right * ex + up * ey;
            org = org + off;
            dir = normalize(dir * g.focus - off);                 // through the point at distance `focus` along the pinhole ray: a spherical surface of focus
        }
    }
    origin = make_float4(org.x, org.y, org.z, 0.0f);
    direction = make_float4(dir.x, dir.y, dir.z, 0.0f);
}

// nullptr, or why bhray_accum_set_camera refuses the struct (include/bhray.h)
const char* still_camera_error(const bhray_still_camera* cam);
// whether the camera is "pinhole, no lens": the accumulation then runs accum_gen_kernel / adapt_gen_kernel, untouched
inline bool still_camera_is_default(const bhray_still_camera& cam) { return cam.projection == BHRAY_STILL_PINHOLE && !(cam.lens_radius > 0.0f); }
// the generators' constants from the ctx's configuration, the camera block of the uniforms and the still camera: derive_frame's operations for right / up / fwd_ff,
// accum_gen_args' for the level.  s0 and k stay 0.
void still_gen_fill(StillGen& g, const bhray_config& cfg, const bhray_camera_uniform& cam, const bhray_still_camera& still);
// records (s - s0) * npix + p of `rays` (two float4 each): the record of sample s through frame pixel p, s = g.a.s0 .. g.a.s0 + g.a.k - 1, as launch_accum_gen.
// k * npix <= 2^26.  Enqueues only.
hipError_t launch_still_gen(const StillGen& g, float4* rays, hipStream_t s);
// records jj * n_active + i: sample issued[p] + j0 + jj through frame pixel p = list[i] (nullptr: i), jj = 0 .. g.a.k - 1, as launch_adapt_gen.  g.a.s0 is not read.
hipError_t launch_still_gen_list(const StillGen& g, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state, float4* rays, hipStream_t s);

}  // namespace bhray
