// bhray_render — minimal C++ host program over renderer.hpp: renders one frame of the reference's default scene
// (camera (0,0,-19), hole at the origin, disk 2..10, R = 20; camera.rs:10-16, blackhole.rs:16-28) and writes the HDR frame
// as raw little-endian f32 RGBA (row 0 = top).  Usage:
//   bhray_render OUT.f32 [--rk] [--base W H] [--levels N] [--disk-size S] [--obj mesh.obj]... [--bvh reference|device] [--pose RX RY RZ] [--lensed-mesh] [--devices 0,1,2,...] [--panorama W H] [--spp N] [--spp-adaptive MIN MAX TOL [--spp-round R] [--spp-dark D]] [--still-camera pinhole|equirect|fisheye FOV] [--lens RADIUS FOCUS] [--filter tent RADIUS|cubic RADIUS B C] [--stars-seeded N SEED] [--observer VX VY VZ [--no-beaming]] [--passes coverage,geometry,position,escape] [--denoise [ITERATIONS]] [--pick X Y] [--path X Y [--path-stride S]]
// --spp N: instead of the ladder's frame, a supersampled still - the mean of N jittered samples per frame pixel, sky resolved, accumulated on the GPU
//   (Renderer::render_still: bhray_accum_*); written the same way.  Not with --devices or --panorama.
// --spp-adaptive MIN MAX TOL [--spp-round R] [--spp-dark D]: an adaptive still instead - every pixel takes MIN samples, then R more (4 by default) for as long as the
//   relative standard error of its mean compressed luminance, with D (0.01 by default) added to the mean, exceeds TOL, and at most MAX
//   (Renderer::render_still_adaptive: bhray_accum_add_adaptive); written the same way, followed by one line
//   adaptive rounds=N rays=N mean_count=F
//   Not with --spp, --devices or --panorama.
// --still-camera pinhole|equirect|fisheye FOV, --lens RADIUS FOCUS (with --spp or --spp-adaptive): the still's camera model, evaluated on the GPU (bhray_accum_set_camera,
//   DESIGN.md §21) - a 360 x 180 degree panorama over the frame, an equidistant fisheye of full opening angle FOV (radians, 0 < FOV <= 2 pi), or the pinhole (the
//   default); --lens gives the pinhole a thin lens of aperture radius RADIUS > 0 focused at distance FOCUS > 0 (depth of field) and goes with no other projection.
// --filter tent RADIUS | cubic RADIUS B C (with --spp; not with --spp-adaptive): the still's pixel reconstruction filter in place of the box (bhray_accum_set_filter,
//   DESIGN.md §22) - a tent of half width RADIUS pixels (0.5 <= RADIUS <= 2.5) or the Mitchell-Netravali cubic with parameters B and C, each in [0, 1], its support
//   scaled to half width RADIUS (1 <= RADIUS <= 2.5).
// --stars-seeded N SEED (with --spp; not with --spp-adaptive or --lens): a seeded catalogue of N point stars (bhusie::star_catalogue, 1 <= N <= BHRAY_MAX_STARS) lensed into
//   every sample's image of the still (bhray_set_stars + bhray_accum_set_stars): pixel-sharp stars at sub-pixel accuracy, --filter their point spread function.
// --observer VX VY VZ [--no-beaming] (with --spp or --spp-adaptive): the still as an observer moving with velocity (VX, VY, VZ) sees it - static frame, world axes, units
//   of c, at most 0.99 - (bhray_accum_set_observer): every look direction is Lorentz-aberrated on the GPU and every sample scaled by the bolometric D^4;
//   --no-beaming keeps the aberration alone.  A zero velocity is no observer.
// --passes LIST (with --spp; not with --spp-adaptive or --panorama): LIST names, separated by commas, the per-pixel maps the still carries beside its colour
//   (bhray_accum_set_passes) - coverage (horizon, disk, mesh shares), geometry (closest approach, iterations, transmittance), position (the disk / mesh hit
//   point, premultiplied by its coverage), escape (the mean escape direction).  Each goes to OUT.f32.<name> as raw f32 RGBA, the format of OUT.f32 itself.
// --denoise [ITERATIONS] (with --spp; not with --spp-adaptive or --panorama): the still is written through the edge-avoiding a-trous filter guided by its passes
//   (bhray_accum_read_denoised) in place of the plain mean; ITERATIONS (1 .. 5, the library's default when left out) levels at tap spacing 1, 2, 4, 8,
//   16 pixels, every other parameter the library's default.  Without --passes the still carries all four passes for it (none is written); with --passes, those.
// --path X Y [--path-stride S]: after the frame, the pick line of pixel (X, Y) and then the light path behind it, one line per point - that pixel's pinhole ray through
//   bhray_trace_rays_paths (Renderer::ray_path), a point every 2^S iterations (S = 0 by default) and the end point:
//   ITERATION X Y Z
// Not with --lensed-mesh (paths under mesh lensing are not built: an error), --devices or --panorama.
// --pick X Y: after the frame, one line with the record of its pixel (X, Y) - that pixel's pinhole ray through bhray_trace_rays_records (Renderer::pick):
//   pick X Y hit=none|horizon|disk|mesh model=M triangle=T position=PX PY PZ iterations=I closest=C transmittance=A
// Not with --devices or --panorama.
// --panorama W H: instead of the pinhole frame, a 360 x 180 degree panorama of W x H pixels from the camera's position, its centre column looking along the camera's forward
// (bhusie::equirect_rays through Renderer::render_rays: bhray_trace_rays); written the same way.  Not with --devices.
// --pose: every --obj mesh is turned by the Euler rotation (RX, RY, RZ) about its own origin on the GPU (bhray_pose_from_euler + bhray_set_model_pose); needs --bvh device.
// --lensed-mesh: the meshes are tested on every step inside the relativity sphere too (bhray_set_mesh_lensing): a mesh inside the sphere is visible.
//   Together with --spp, --spp-adaptive (and their --still-camera, --lens, --filter, --stars-seeded), --panorama or --pick the ray batches behind those are lensed too
//   (Renderer::lens_ray_batches: BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS): the still, the panorama and the picked record show the lensed mesh.
// --bvh device: every mesh's tree is built on the GPU (bhray_upload_model_build) instead of by the reference's host builder (the default).
// --obj: repeatable; the i-th mesh goes to model slot i (Renderer::add_model), at the position its OBJ loader gives it.
// --devices: row-tile the frame over several GPUs from this one process (RCCL gather to the first one, inside libbhray).
//   bhray_render --handoff sync|hdr|sky|sky1|sky-temporal|display FRAMES OUT.bin [--rk] [--base W H] [--levels N] [--sky-filter] [--stars-seeded N SEED]
//   bhray_render --dropin FRAMES [--rk] [--base W H] [--levels N]
// --handoff: FRAMES frames of the same scene (time += 1/60 per frame) through Renderer::render_handoff in the given form, every DELIVERED frame
// appended to OUT.bin in delivery order (RGBA32F for sync / hdr, RGBA16F for sky, RGBA8 sRGB for display) - the tests compare them with the frames the Python host renders.
// --sky-filter (with --handoff): the sky pass of the sky and display forms is the footprint-filtered one (bhray_set_sky_filter).
// --stars-seeded N SEED (with --handoff): the sky pass of the sky and display forms receives a seeded catalogue of N point stars (bhusie::star_catalogue through
//   RayPipeline::set_stars: bhray_set_stars), 1 <= N <= BHRAY_MAX_STARS.
// --dropin: times the drop-in shim of INTEGRATION.md §3 the way the reference host drives it - one thread, `time += dt` every frame
// (mod.rs:382), every frame handed to host memory - in its three hand-off forms, and prints one JSON object (bench.py embeds it as `dropin`).
// Textures: the disk texture comes from the reference's own generator (bhray_generate_disk_texture); the LUT and the sky
// are flat grey here (this program demonstrates the host surface, the tests use the seeded assets).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "renderer.hpp"

namespace {
// seeded stand-ins of the image assets (color.png is an image, sky.png is missing from the reference checkout): a smooth LUT and a
// noisy sky of the shipped sizes, so that the texture taps of the timed frames touch real memory
void fill_textures(bhusie::RayPipeline& rp, uint32_t disk) {
    std::vector<uint8_t> d((size_t)disk * disk * 4);
    bhusie::check(bhray_generate_disk_texture(disk, d.data()));
    rp.set_texture(BHRAY_TEX_DISK, d.data(), disk, disk);
    std::vector<uint8_t> lut(256 * 256 * 4);
    for (int y = 0; y < 256; y++) for (int x = 0; x < 256; x++) {
        uint8_t* p = &lut[((size_t)y * 256 + x) * 4];
        p[0] = (uint8_t)(255 - x / 2); p[1] = (uint8_t)(80 + x / 2); p[2] = (uint8_t)x; p[3] = 255;
    }
    rp.set_texture(BHRAY_TEX_TEMP_LUT, lut.data(), 256, 256);
    std::vector<uint8_t> sky((size_t)4096 * 2048 * 4);
    uint32_t h = 2463534242u;
    for (size_t i = 0; i < sky.size(); i += 4) { h ^= h << 13; h ^= h >> 17; h ^= h << 5; sky[i] = (uint8_t)(h & 63); sky[i + 1] = (uint8_t)((h >> 8) & 63); sky[i + 2] = (uint8_t)((h >> 16) & 127); sky[i + 3] = 255; }
    rp.set_texture(BHRAY_TEX_SKY, sky.data(), 4096, 2048);
}

struct Leg { const char* name; bhusie::Handoff h; uint32_t in_flight; bool temporal; bool orbit; };

// one leg: `frames` frames through Renderer::render_handoff, host wall clock around them (after a warm-up of 8 frames)
double run_leg(const Leg& L, uint32_t bw, uint32_t bh, uint32_t levels, bool rk, int frames, uint64_t* checksum, uint32_t* w, uint32_t* h) {
    bhusie::Renderer r({bw, bh}, 3, levels, 0, L.in_flight, L.h, L.temporal);
    fill_textures(r.ray_pipeline(), 1000);
    r.ray_details.integration_method = rk ? 1 : 0;
    auto res = r.ray_pipeline().resolution(); *w = res.first; *h = res.second;
    const size_t words = (size_t)res.first * res.second * (L.h == bhusie::Handoff::AsyncSky ? 2 : 4);
    auto frame = [&](int i) {
        if (L.orbit) {                                   // a camera orbiting the hole, 0.02 rad per frame, looking at it (the UI's drag speed)
            const float a = 0.02f * (float)i;
            r.camera.position[0] = 19.0f * std::sin(a); r.camera.position[1] = 0.0f; r.camera.position[2] = -19.0f * std::cos(a);
            r.camera.forward[0] = -std::sin(a); r.camera.forward[1] = 0.0f; r.camera.forward[2] = std::cos(a);
        }
        const uint32_t* px = (const uint32_t*)r.render_handoff(1.0f / 60.0f);
        if (px) *checksum += px[(size_t)i * 7919 % words];          // the host touches what it was handed
    };
    for (int i = 0; i < 8; i++) frame(i);
    bhusie::check(bhray_sync(r.ray_pipeline().ctx()), r.ray_pipeline().ctx());
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < frames; i++) frame(8 + i);
    r.ray_pipeline().drain();
    bhusie::check(bhray_sync(r.ray_pipeline().ctx()), r.ray_pipeline().ctx());
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

int main(int argc, char** argv) {
    if (argc >= 5 && !std::strcmp(argv[1], "--handoff")) {
        const char* form = argv[2]; const int frames = std::atoi(argv[3]); const char* out_path = argv[4];
        uint32_t bw = 24, bh = 14, levels = 3; bool rk = false, sky_filter = false;
        long stars_n = 0, stars_seed = 0;
        for (int i = 5; i < argc; i++) {
            if (!std::strcmp(argv[i], "--rk")) rk = true;
            else if (!std::strcmp(argv[i], "--sky-filter")) sky_filter = true;
            else if (!std::strcmp(argv[i], "--stars-seeded")) {
                char *e1 = nullptr, *e2 = nullptr;
                if (i + 2 >= argc) { std::fprintf(stderr, "--stars-seeded needs N and SEED\n"); return 2; }
                stars_n = std::strtol(argv[++i], &e1, 10); stars_seed = std::strtol(argv[++i], &e2, 10);
                if (*e1 || *e2 || stars_n < 1 || stars_n > (long)BHRAY_MAX_STARS || stars_seed < 0) { std::fprintf(stderr, "--stars-seeded needs 1 <= N <= %u and SEED >= 0\n", BHRAY_MAX_STARS); return 2; }
            }
            else if (!std::strcmp(argv[i], "--base") && i + 2 < argc) { bw = (uint32_t)std::atoi(argv[++i]); bh = (uint32_t)std::atoi(argv[++i]); }
            else if (!std::strcmp(argv[i], "--levels") && i + 1 < argc) levels = (uint32_t)std::atoi(argv[++i]);
        }
        try {
            const bool sky = !std::strncmp(form, "sky", 3), temporal = !std::strcmp(form, "sky-temporal"), display = !std::strcmp(form, "display");
            const bhusie::Handoff h = !std::strcmp(form, "sync") ? bhusie::Handoff::Sync
                                    : (display ? bhusie::Handoff::AsyncDisplay : (sky ? bhusie::Handoff::AsyncSky : bhusie::Handoff::AsyncHdr));
            const uint32_t in_flight = (h == bhusie::Handoff::Sync || !std::strcmp(form, "sky1")) ? 1u : 2u;   // sky1: the sky form, one frame in flight
            bhusie::Renderer r({bw, bh}, 3, levels, 0, in_flight, h, temporal);
            fill_textures(r.ray_pipeline(), 128);
            if (sky_filter) r.ray_pipeline().set_sky_filter(true);
            if (stars_n > 0) r.ray_pipeline().set_stars(bhusie::star_catalogue((uint32_t)stars_n, (uint32_t)stars_seed));
            r.ray_details.integration_method = rk ? 1 : 0;
            auto res = r.ray_pipeline().resolution();
            const size_t bytes = (size_t)res.first * res.second * (display ? 4 : (sky ? 8 : 16));
            FILE* f = std::fopen(out_path, "wb");
            if (!f) { std::perror(out_path); return 1; }
            int delivered = 0;
            for (int i = 0; i < frames; i++) {
                const void* px = r.render_handoff(1.0f / 60.0f);
                if (px) { std::fwrite(px, 1, bytes, f); delivered++; }
            }
            // the frames still in flight: one more finish() per frame (the host would show them on its next frames)
            for (uint32_t k = 1; k < in_flight; k++) {
                r.ray_pipeline().drain();
                const void* px = r.ray_pipeline().finish_pending(k);
                if (px) { std::fwrite(px, 1, bytes, f); delivered++; }
            }
            std::fclose(f);
            std::printf("%ux%u %d\n", res.first, res.second, delivered);
        } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "--dropin")) {
        const int frames = std::atoi(argv[2]);
        uint32_t bw = 72, bh = 41, levels = 4; bool rk = false;
        for (int i = 3; i < argc; i++) {
            if (!std::strcmp(argv[i], "--rk")) rk = true;
            else if (!std::strcmp(argv[i], "--base") && i + 2 < argc) { bw = (uint32_t)std::atoi(argv[++i]); bh = (uint32_t)std::atoi(argv[++i]); }
            else if (!std::strcmp(argv[i], "--levels") && i + 1 < argc) levels = (uint32_t)std::atoi(argv[++i]);
        }
        const Leg legs[] = {
            {"sync_read_hdr", bhusie::Handoff::Sync, 1, false, false},
            {"async_rgba32f_2_in_flight", bhusie::Handoff::AsyncHdr, 2, false, false},
            {"async_sky_rgba16f_2_in_flight", bhusie::Handoff::AsyncSky, 2, false, false},
            {"async_sky_rgba16f_2_in_flight_temporal", bhusie::Handoff::AsyncSky, 2, true, false},
            {"async_sky_rgba16f_2_in_flight_temporal_orbit", bhusie::Handoff::AsyncSky, 2, true, true},
            {"async_sky_rgba16f_2_in_flight_orbit", bhusie::Handoff::AsyncSky, 2, false, true},
        };
        try {
            std::printf("{\"frames\": %d, \"integrator\": \"%s\", \"legs\": {", frames, rk ? "rk" : "euler");
            uint64_t checksum = 0; uint32_t w = 0, h = 0; bool first = true;
            for (const Leg& L : legs) {
                if (L.temporal && levels > BHRAY_MAX_SPEC_LEVELS) continue;
                const double s = run_leg(L, bw, bh, levels, rk, frames, &checksum, &w, &h);
                std::printf("%s\"%s\": {\"ms_per_frame\": %.5f, \"mrays_per_s\": %.2f, \"frames_in_flight\": %u}", first ? "" : ", ", L.name, s / frames * 1e3,
                            (double)w * h * frames / s / 1e6, L.in_flight);
                first = false;
            }
            std::printf("}, \"frame\": [%u, %u], \"checksum\": %llu}\n", w, h, (unsigned long long)checksum);
        } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
        return 0;
    }
    if (argc < 2) { std::fprintf(stderr, "usage: %s OUT.f32 [--rk] [--base W H] [--levels N] [--disk-size S] [--obj mesh.obj]... [--bvh reference|device] [--pose RX RY RZ] [--lensed-mesh] [--devices 0,1,...] [--panorama W H] [--spp N] [--spp-adaptive MIN MAX TOL [--spp-round R] [--spp-dark D]] [--still-camera pinhole|equirect|fisheye FOV] [--lens RADIUS FOCUS] [--filter tent RADIUS|cubic RADIUS B C] [--stars-seeded N SEED] [--observer VX VY VZ [--no-beaming]] [--passes coverage,geometry,position,escape] [--denoise [ITERATIONS]] [--pick X Y] [--path X Y [--path-stride S]]\n", argv[0]); return 2; }
    uint32_t bw = 72, bh = 41, levels = 4, disk = 256, pano_w = 0, pano_h = 0;
    long pick_x = -1, pick_y = -1, path_x = -1, path_y = -1, path_stride = 0, spp = 0;
    bool rk = false, bvh_device = false, lensed = false, posed = false, adaptive = false;
    long a_min = 0, a_max = 0, a_round = 4, stars_n = 0, stars_seed = 0;
    double a_tol = 0.0, a_dark = 0.01;
    bool still_given = false, lens_given = false, filter_given = false, observer_given = false, no_beaming = false;
    uint32_t passes = 0;
    bool passes_given = false, denoise_given = false;
    bhray_still_denoise denoise{};
    bhray_still_denoise_default(&denoise);
    static const struct { const char* name; uint32_t bit; } pass_names[] = {{"coverage", BHRAY_PASS_COVERAGE}, {"geometry", BHRAY_PASS_GEOMETRY}, {"position", BHRAY_PASS_POSITION}, {"escape", BHRAY_PASS_ESCAPE}};
    bhray_observer observer{};
    bhray_observer_default(&observer);
    bhray_still_filter filter{};
    bhray_still_filter_default(&filter);
    bhray_still_camera still{};
    bhray_still_camera_default(&still);
    float rotation[3] = {0.0f, 0.0f, 0.0f};
    std::vector<const char*> objs;
    std::vector<int> devices;
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "--rk")) rk = true;
        else if (!std::strcmp(argv[i], "--base") && i + 2 < argc) { bw = (uint32_t)std::atoi(argv[++i]); bh = (uint32_t)std::atoi(argv[++i]); }
        else if (!std::strcmp(argv[i], "--levels") && i + 1 < argc) levels = (uint32_t)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--disk-size") && i + 1 < argc) disk = (uint32_t)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--obj") && i + 1 < argc) objs.push_back(argv[++i]);
        else if (!std::strcmp(argv[i], "--bvh") && i + 1 < argc && (!std::strcmp(argv[i + 1], "device") || !std::strcmp(argv[i + 1], "reference"))) bvh_device = !std::strcmp(argv[++i], "device");
        else if (!std::strcmp(argv[i], "--pose") && i + 3 < argc) { posed = true; for (int a = 0; a < 3; a++) rotation[a] = (float)std::atof(argv[++i]); }
        else if (!std::strcmp(argv[i], "--lensed-mesh")) lensed = true;
        else if (!std::strcmp(argv[i], "--panorama") && i + 2 < argc) { pano_w = (uint32_t)std::atoi(argv[++i]); pano_h = (uint32_t)std::atoi(argv[++i]); if (pano_w < 1 || pano_h < 1) { std::fprintf(stderr, "--panorama needs W >= 1 and H >= 1\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--spp") && i + 1 < argc) { spp = std::atol(argv[++i]); if (spp < 1 || spp > (long)BHRAY_ACCUM_MAX_SAMPLES) { std::fprintf(stderr, "--spp needs 1 <= N <= %u\n", BHRAY_ACCUM_MAX_SAMPLES); return 2; } }
        else if (!std::strcmp(argv[i], "--spp-adaptive") && i + 3 < argc) {
            adaptive = true; a_min = std::atol(argv[++i]); a_max = std::atol(argv[++i]); a_tol = std::atof(argv[++i]);
            if (a_min < 2 || a_max < a_min || a_max > (long)BHRAY_ACCUM_MAX_SAMPLES) { std::fprintf(stderr, "--spp-adaptive needs 2 <= MIN <= MAX <= %u\n", BHRAY_ACCUM_MAX_SAMPLES); return 2; }
            if (!std::isfinite(a_tol) || a_tol < 0.0) { std::fprintf(stderr, "--spp-adaptive needs a finite TOL >= 0\n"); return 2; }
        }
        else if (!std::strcmp(argv[i], "--spp-round") && i + 1 < argc) { a_round = std::atol(argv[++i]); if (a_round < 1 || a_round > (long)BHRAY_ACCUM_MAX_SAMPLES) { std::fprintf(stderr, "--spp-round needs 1 <= R <= %u\n", BHRAY_ACCUM_MAX_SAMPLES); return 2; } }
        else if (!std::strcmp(argv[i], "--spp-dark") && i + 1 < argc) { a_dark = std::atof(argv[++i]); if (!std::isfinite(a_dark) || a_dark < 0.0) { std::fprintf(stderr, "--spp-dark needs a finite D >= 0\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--still-camera") && i + 1 < argc) {
            const char* kind = argv[++i];
            still_given = true;
            if (!std::strcmp(kind, "pinhole")) still.projection = BHRAY_STILL_PINHOLE;
            else if (!std::strcmp(kind, "equirect")) still.projection = BHRAY_STILL_EQUIRECT;
            else if (!std::strcmp(kind, "fisheye") && i + 1 < argc) {
                still.projection = BHRAY_STILL_FISHEYE;
                const double fov = std::atof(argv[++i]);
                if (!std::isfinite(fov) || !(fov > 0.0) || (float)fov > 6.28318548f) { std::fprintf(stderr, "--still-camera fisheye needs 0 < FOV <= 2 pi (radians)\n"); return 2; }
                still.fisheye_fov = (float)fov;
            }
            else { std::fprintf(stderr, "--still-camera needs pinhole, equirect or fisheye FOV\n"); return 2; }
        }
        else if (!std::strcmp(argv[i], "--lens") && i + 2 < argc) {
            const double radius = std::atof(argv[++i]), focus = std::atof(argv[++i]);
            if (!std::isfinite(radius) || !(radius > 0.0) || !std::isfinite(focus) || !(focus > 0.0)) { std::fprintf(stderr, "--lens needs RADIUS > 0 and FOCUS > 0\n"); return 2; }
            lens_given = true; still.lens_radius = (float)radius; still.focus_distance = (float)focus;
        }
        else if (!std::strcmp(argv[i], "--filter") && i + 1 < argc) {
            const char* kind = argv[++i];
            filter_given = true;
            if (!std::strcmp(kind, "tent") && i + 1 < argc) {
                const double radius = std::atof(argv[++i]);
                if (!std::isfinite(radius) || (float)radius < 0.5f || (float)radius > 2.5f) { std::fprintf(stderr, "--filter tent needs 0.5 <= RADIUS <= 2.5 (pixels)\n"); return 2; }
                filter.kind = BHRAY_FILTER_TENT; filter.radius = (float)radius;
            }
            else if (!std::strcmp(kind, "cubic") && i + 3 < argc) {
                const double radius = std::atof(argv[++i]), b = std::atof(argv[++i]), c = std::atof(argv[++i]);
                if (!std::isfinite(radius) || (float)radius < 1.0f || (float)radius > 2.5f) { std::fprintf(stderr, "--filter cubic needs 1 <= RADIUS <= 2.5 (pixels)\n"); return 2; }
                if (!std::isfinite(b) || (float)b < 0.0f || (float)b > 1.0f || !std::isfinite(c) || (float)c < 0.0f || (float)c > 1.0f) { std::fprintf(stderr, "--filter cubic needs B and C in [0, 1]\n"); return 2; }
                filter.kind = BHRAY_FILTER_CUBIC; filter.radius = (float)radius; filter.b = (float)b; filter.c = (float)c;
            }
            else { std::fprintf(stderr, "--filter needs tent RADIUS or cubic RADIUS B C\n"); return 2; }
        }
        else if (!std::strcmp(argv[i], "--stars-seeded")) {
            char *e1 = nullptr, *e2 = nullptr;
            if (i + 2 >= argc) { std::fprintf(stderr, "--stars-seeded needs N and SEED\n"); return 2; }
            stars_n = std::strtol(argv[++i], &e1, 10); stars_seed = std::strtol(argv[++i], &e2, 10);
            if (*e1 || *e2 || stars_n < 1 || stars_n > (long)BHRAY_MAX_STARS || stars_seed < 0) { std::fprintf(stderr, "--stars-seeded needs 1 <= N <= %u and SEED >= 0\n", BHRAY_MAX_STARS); return 2; }
        }
        else if (!std::strcmp(argv[i], "--observer") && i + 3 < argc) {
            observer_given = true;
            for (int a = 0; a < 3; a++) observer.velocity[a] = (float)std::atof(argv[++i]);
            const float* v = observer.velocity;
            if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2]) || (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > BHRAY_OBSERVER_MAX_SPEED2) {
                std::fprintf(stderr, "--observer needs a finite velocity of at most 0.99 (units of c)\n"); return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--no-beaming")) no_beaming = true;
        else if (!std::strcmp(argv[i], "--passes") && i + 1 < argc) {
            passes_given = true;
            const std::string list = argv[++i];
            for (size_t a = 0; a <= list.size();) {
                const size_t e = std::min(list.find(',', a), list.size());
                const std::string name = list.substr(a, e - a);
                uint32_t bit = 0;
                for (const auto& pn : pass_names) if (name == pn.name) bit = pn.bit;
                if (!bit) { std::fprintf(stderr, "--passes needs a comma-separated list of coverage, geometry, position, escape\n"); return 2; }
                passes |= bit;
                a = e + 1;
            }
        }
        else if (!std::strcmp(argv[i], "--denoise")) {
            denoise_given = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                const long n = std::atol(argv[++i]);
                if (n < 1 || n > (long)BHRAY_DENOISE_MAX_ITERATIONS) { std::fprintf(stderr, "--denoise needs 1 <= ITERATIONS <= %u\n", BHRAY_DENOISE_MAX_ITERATIONS); return 2; }
                denoise.iterations = (uint32_t)n;
            }
        }
        else if (!std::strcmp(argv[i], "--pick") && i + 2 < argc) { pick_x = std::atol(argv[++i]); pick_y = std::atol(argv[++i]); if (pick_x < 0 || pick_y < 0) { std::fprintf(stderr, "--pick needs X >= 0 and Y >= 0\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--path") && i + 2 < argc) { path_x = std::atol(argv[++i]); path_y = std::atol(argv[++i]); if (path_x < 0 || path_y < 0) { std::fprintf(stderr, "--path needs X >= 0 and Y >= 0\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--path-stride") && i + 1 < argc) { path_stride = std::atol(argv[++i]); if (path_stride < 0 || path_stride > BHRAY_MAX_PATH_STRIDE_LOG2) { std::fprintf(stderr, "--path-stride needs 0 <= S <= %d\n", BHRAY_MAX_PATH_STRIDE_LOG2); return 2; } }
        else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) { for (const char* p = argv[++i]; *p; ) { devices.push_back(std::atoi(p)); while (*p && *p != ',') p++; if (*p) p++; } }
        else { std::fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    if (adaptive && spp) { std::fprintf(stderr, "--spp-adaptive and --spp are two ways to fill the same image: give one\n"); return 2; }
    if (adaptive && pano_w) { std::fprintf(stderr, "--spp-adaptive samples the pixels of the pinhole frame: not with --panorama\n"); return 2; }
    if (adaptive && (a_max - a_min) % a_round != 0) { std::fprintf(stderr, "--spp-adaptive needs MAX - MIN to be a multiple of the round (--spp-round, 4 by default)\n"); return 2; }
    if ((still_given || lens_given) && !spp && !adaptive) { std::fprintf(stderr, "--still-camera and --lens are the camera of a still: give --spp or --spp-adaptive\n"); return 2; }
    if (filter_given && adaptive) { std::fprintf(stderr, "--filter weighs sample s of a pixel's neighbours: not with --spp-adaptive, whose pixels take different samples\n"); return 2; }
    if (filter_given && !spp) { std::fprintf(stderr, "--filter is the reconstruction filter of a still: give --spp\n"); return 2; }
    if (stars_n && adaptive) { std::fprintf(stderr, "--stars-seeded lights a pixel from sample s of its neighbours: not with --spp-adaptive, whose pixels take different samples\n"); return 2; }
    if (stars_n && lens_given) { std::fprintf(stderr, "--stars-seeded needs footprints: not with --lens, whose neighbouring pixels look through different lens points\n"); return 2; }
    if (stars_n && !spp) { std::fprintf(stderr, "--stars-seeded in this mode is the star field of a still: give --spp\n"); return 2; }
    if (observer_given && !spp && !adaptive) { std::fprintf(stderr, "--observer is the observer of a still: give --spp or --spp-adaptive\n"); return 2; }
    if (passes_given && adaptive) { std::fprintf(stderr, "--passes sums every sample of a launch's pixels: not with --spp-adaptive, whose adder works over a pixel list\n"); return 2; }
    if (passes_given && pano_w) { std::fprintf(stderr, "--passes are the maps of a still over the pinhole frame: not with --panorama\n"); return 2; }
    if (passes_given && !spp) { std::fprintf(stderr, "--passes are the maps of a still: give --spp\n"); return 2; }
    if (denoise_given && adaptive) { std::fprintf(stderr, "--denoise is guided by the passes of a still: not with --spp-adaptive, which carries none\n"); return 2; }
    if (denoise_given && pano_w) { std::fprintf(stderr, "--denoise filters a still over the pinhole frame: not with --panorama\n"); return 2; }
    if (denoise_given && !spp) { std::fprintf(stderr, "--denoise filters a still: give --spp\n"); return 2; }
    if (no_beaming && !observer_given) { std::fprintf(stderr, "--no-beaming goes with --observer\n"); return 2; }
    if (lens_given && still.projection != BHRAY_STILL_PINHOLE) { std::fprintf(stderr, "--lens goes with the pinhole projection only\n"); return 2; }
    if (spp && pano_w) { std::fprintf(stderr, "--spp samples the pixels of the pinhole frame: not with --panorama\n"); return 2; }
    if (path_x >= 0 && pano_w) { std::fprintf(stderr, "--path names a pixel of the pinhole frame: not with --panorama\n"); return 2; }
    if (pick_x >= 0 && pano_w) { std::fprintf(stderr, "--pick names a pixel of the pinhole frame: not with --panorama\n"); return 2; }
    if (path_x >= 0 && lensed) { std::fprintf(stderr, "--path under --lensed-mesh is not built (bhray_trace_rays_paths is refused while mesh lensing is on)\n"); return 2; }
    if (posed && !bvh_device) { std::fprintf(stderr, "--pose needs --bvh device (a pose is applied to a tree built on the GPU)\n"); return 2; }
    try {
        std::unique_ptr<bhusie::Renderer> rp(devices.empty() ? new bhusie::Renderer({bw, bh}, 3, levels) : new bhusie::Renderer({bw, bh}, 3, levels, devices));
        bhusie::Renderer& r = *rp;
        std::vector<uint8_t> d((size_t)disk * disk * 4);
        bhusie::check(bhray_generate_disk_texture(disk, d.data()));
        r.ray_pipeline().set_texture(BHRAY_TEX_DISK, d.data(), disk, disk);
        const uint8_t grey[4] = {160, 160, 160, 255};
        r.ray_pipeline().set_texture(BHRAY_TEX_TEMP_LUT, grey, 1, 1);
        r.ray_pipeline().set_texture(BHRAY_TEX_SKY, grey, 1, 1);
        std::vector<bhusie::Model> models;
        for (const char* obj : objs) { models.emplace_back(obj); r.add_model(models.back(), bvh_device); }
        if (posed) {
            const float pivot[3] = {0.0f, 0.0f, 0.0f};
            float pose[12];
            bhusie::check(bhray_pose_from_euler(rotation, pivot, 1.0f, pose));
            for (uint32_t i = 0; i < (uint32_t)models.size(); i++) r.ray_pipeline().set_model_pose(i, pose);
        }
        r.ray_details.integration_method = rk ? 1 : 0;
        r.mesh_lensing = lensed;
        r.lens_ray_batches = lensed && (spp || adaptive || pano_w || pick_x >= 0);        // the stills, the panorama and the pick trace ray batches: lensed too (BHRAY_LENS_RAYS)
        if (observer_given) { observer.beaming = no_beaming ? 0u : 1u; r.observer = observer; }
        r.still_passes = denoise_given && !passes ? (uint32_t)BHRAY_PASS_ALL : passes;
        std::vector<float> out;
        std::vector<uint32_t> counts;
        bhray_accum_adaptive_info ainfo{};
        auto res = r.ray_pipeline().resolution();
        if (pano_w) {
            out = r.render_rays(bhusie::equirect_rays(r.camera.position, r.camera.forward, pano_w, pano_h));
            res = {pano_w, pano_h};
        } else if (adaptive) {
            bhray_accum_adaptive a{};
            a.min_samples = (uint32_t)a_min; a.max_samples = (uint32_t)a_max; a.round_samples = (uint32_t)a_round; a.tolerance = (float)a_tol; a.dark = (float)a_dark;
            out = r.render_still_adaptive(a, &ainfo, &counts, &still);
        } else if (spp) {
            if (stars_n > 0) r.ray_pipeline().set_stars(bhusie::star_catalogue((uint32_t)stars_n, (uint32_t)stars_seed));
            out = r.render_still((uint32_t)spp, &still, filter_given ? &filter : nullptr, stars_n > 0);
            if (denoise_given) out = r.still_denoised(&denoise);   // in place of the plain mean
        } else {
            r.render(0.0f);
            out = r.ray_pipeline().output();
        }
        FILE* f = std::fopen(argv[1], "wb");
        if (!f) { std::perror(argv[1]); return 1; }
        std::fwrite(out.data(), sizeof(float), out.size(), f);
        std::fclose(f);
        for (const auto& pn : pass_names) {                        // the still's passes beside it: OUT.<name>, the same raw floats
            if (!(passes & pn.bit)) continue;
            const std::string path = std::string(argv[1]) + "." + pn.name;
            const std::vector<float> plane = r.still_pass(pn.bit);
            FILE* g = std::fopen(path.c_str(), "wb");
            if (!g) { std::perror(path.c_str()); return 1; }
            std::fwrite(plane.data(), sizeof(float), plane.size(), g);
            std::fclose(g);
        }
        std::printf("%ux%u\n", res.first, res.second);
        if (adaptive) {
            double total = 0.0;
            for (uint32_t n : counts) total += (double)n;
            std::printf("adaptive rounds=%u rays=%llu mean_count=%.6f\n", ainfo.rounds, (unsigned long long)ainfo.rays, counts.empty() ? 0.0 : total / (double)counts.size());
        }
        auto print_pick = [](long pick_x, long pick_y, const bhray_ray_record& p) {
            const uint32_t kind = p.hit & 0xffu;
            const char* name = kind == BHRAY_HIT_NONE ? "none" : kind == BHRAY_HIT_HORIZON ? "horizon" : kind == BHRAY_HIT_DISK ? "disk" : kind == BHRAY_HIT_MESH ? "mesh" : "unusable";
            std::printf("pick %ld %ld hit=%s model=%d triangle=%d position=%.9g %.9g %.9g iterations=%u closest=%.9g transmittance=%.9g\n", pick_x, pick_y, name,
                        kind == BHRAY_HIT_MESH ? (int)((p.hit >> 8) & 0xffu) : -1, (int)p.triangle, p.position[0], p.position[1], p.position[2], p.iterations, p.closest, p.transmittance);
        };
        if (pick_x >= 0) print_pick(pick_x, pick_y, r.pick((uint32_t)pick_x, (uint32_t)pick_y));
        if (path_x >= 0) {
            const auto path = r.ray_path((uint32_t)path_x, (uint32_t)path_y, (uint32_t)path_stride);
            print_pick(path_x, path_y, path.record);
            for (const bhray_path_point& q : path.points) std::printf("%u %.9g %.9g %.9g\n", q.iteration, q.position[0], q.position[1], q.position[2]);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
