// renderer.hpp — C++ host-side mirror of the reference's ray-pass surface, over the C ABI (include/bhray.h).
//
// The reference host is Rust; with no Rust toolchain in this image the host side above the C ABI is C++.  Names and
// argument meaning follow the Rust:
//   RayDetails            src/renderer/pipelines/ray_pipeline.rs:3-14   (defaults: src/renderer/mod.rs:116-121)
//   Camera / BlackHole    src/scene/camera.rs:3-16, src/scene/blackhole.rs:3-28
//   Model, load_model     src/renderer/triangle.rs:65-259, src/renderer/model.rs:7-87
//   RayPipeline           src/renderer/pipelines/ray_pipeline.rs:28-310  {new, pass, output_view}
//   Renderer              src/renderer/mod.rs:58-207, 370-420            {new, render} restricted to the ray pass
// Header-only; link with -lbhray.  Errors become std::runtime_error (the reference panics).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/bhray.h"

namespace bhusie {

inline void check(int rc, const bhray_ctx* ctx = nullptr) {
    if (rc != BHRAY_OK) {
        const char* m = bhray_last_error(ctx);
        throw std::runtime_error(std::string("bhray: ") + ((m && *m) ? m : bhray_strerror(rc)));
    }
}

// A seeded catalogue of point stars for RayPipeline::set_stars: directions uniform on the sphere (Marsaglia's method, the rejected draws re-hashed), fluxes a power
// law flux_min / t^2 with t uniform in [1/32, 1), a warm-to-cool tint.  Binary64 + - * / sqrt on hashed integers, then one rounding to binary32: the bytes of the
// Python host's assets.star_catalogue(n, seed).
inline uint32_t star_hash(uint32_t x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
inline std::vector<bhray_star> star_catalogue(uint32_t n, uint32_t seed, double flux_min = 2e-7) {
    std::vector<bhray_star> out(n);
    const double u24 = 1.0 / 16777216.0;
    for (uint32_t i = 0; i < n; i++) {
        bhray_star s = {{0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, 0.0f}};
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t h0 = star_hash(i * 0x9E3779B1u ^ star_hash(seed * 7919u + 13u + k));
            const uint32_t h1 = star_hash(h0 ^ 0x68E31DA4u), h2 = star_hash(h1 ^ 0xB5297A4Du), h3 = star_hash(h2 ^ 0x1B56C4E9u);
            const double x1 = (double)(h0 >> 8) * u24 * 2.0 - 1.0, x2 = (double)(h1 >> 8) * u24 * 2.0 - 1.0;
            const double q = x1 * x1 + x2 * x2;
            if (!(q < 1.0)) continue;
            const double r = std::sqrt(1.0 - q);
            const double t = 1.0 - (double)(h2 >> 8) * u24 * (31.0 / 32.0);
            const double f = flux_min / (t * t);
            const double tint = (double)(h3 >> 8) * u24;
            s.dir[0] = (float)(2.0 * x1 * r); s.dir[1] = (float)(2.0 * x2 * r); s.dir[2] = (float)(1.0 - 2.0 * q);
            s.flux[0] = (float)(f * (0.85 + 0.15 * tint)); s.flux[1] = (float)(f * 0.9); s.flux[2] = (float)(f * (1.0 - 0.15 * tint));
            break;
        }
        out[i] = s;
    }
    return out;
}

struct RayDetails : bhray_details {
    RayDetails() { bhray_details_default(this); }              // step_size 0.15, max_iterations 2000, threshold 0.02, Euler
};

struct Camera {                                                // camera.rs:10-16
    float position[3] = {0.0f, 0.0f, -19.0f};
    float forward[3] = {0.0f, 0.0f, 1.0f};
    float fov = 1.0f;
    bhray_camera_uniform uniform() const { bhray_camera_uniform u; bhray_camera_uniform_update(&u, position, forward, fov); return u; }
};

struct BlackHole : bhray_black_hole {                          // blackhole.rs:16-28
    BlackHole() { bhray_black_hole_default(this); }
    bhray_black_hole_uniform uniform() const { bhray_black_hole_uniform u; bhray_black_hole_uniform_update(&u, this); return u; }
};

class Model {                                                  // triangle.rs:65-259
public:
    Model() { check(bhray_model_new(&m_)); }
    explicit Model(const std::string& obj_path) { check(bhray_load_model(obj_path.c_str(), &m_)); }     // model::load_model
    Model(Model&& o) noexcept : m_(o.m_) { o.m_ = nullptr; }
    Model(const Model&) = delete;
    ~Model() { bhray_model_free(m_); }
    void add_vertex(const float p[4]) { check(bhray_model_add_vertex(m_, p)); }
    void add_normal(const float n[4]) { check(bhray_model_add_normal(m_, n)); }
    void add_triangle(const bhray_triangle& t) { check(bhray_model_add_triangle(m_, &t)); }
    void build_bvh() { check(bhray_model_build_bvh(m_)); }
    bhray_model_desc desc() const { bhray_model_desc d; check(bhray_model_desc_get(m_, &d)); return d; }
    const bhray_model* handle() const { return m_; }
private:
    bhray_model* m_ = nullptr;
};

// How a frame reaches a consumer that is not a HIP client of this GPU (the reference's SkyPipeline samples the ray output as a wgpu
// texture, ray_pipeline.rs:297-299, mod.rs:215) - the three forms of the drop-in shim of INTEGRATION.md §3:
enum class Handoff {
    Sync,        // finish() = bhray_read_hdr of the frame just rendered: the naive binding, one frame at a time
    AsyncHdr,    // pass() also enqueues the RGBA32F copy into pinned memory (bhray_read_hdr_async); finish() hands over the OLDEST frame in flight
    AsyncSky,    // pass() also runs the sky pass in the library (sky.wgsl) and enqueues the copy of its RGBA16F image: half the bytes
    AsyncDisplay // pass() also runs the display pass (bloom, mix, ACES, FXAA: DESIGN.md §10) and enqueues the copy of its RGBA8 sRGB image:
                 // the finished picture, a quarter of the RGBA32F bytes - the host uploads it raw into the texture its ScreenPipeline samples
};

// The chain of RayPipelines of one frame (mod.rs:181-207) as one object.
class RayPipeline {
public:
    // RayPipeline::new x levels: base resolution, multiplier, iterations as in mod.rs:177-205
    // frames_in_flight / frames_per_batch > 1: a host that renders ahead (offline sequences); pass() then only stages a frame
    // until a batch is full, output()/flush() launch what is staged
    RayPipeline(std::pair<uint32_t, uint32_t> base, uint32_t multiplier, uint32_t levels, int device = 0, uint32_t frames_in_flight = 1,
                uint32_t frames_per_batch = 1) {
        std::memset(&cfg_, 0, sizeof cfg_);
        check(bhray_ladder_from_base(base.first, base.second, multiplier, levels, &cfg_));
        cfg_.device = device; cfg_.frames_in_flight = frames_in_flight; cfg_.frames_per_batch = frames_per_batch;
        check(bhray_create(&cfg_, &ctx_));
    }
    // Row-tiled over several GPUs of the node, still ONE pipeline object driven from one thread (mod.rs:415-420): partition i
    // of the frame is rendered on devices[i]; pass() also enqueues the RCCL gather to devices[0] and the de-interleave, and
    // output() is the whole frame.
    RayPipeline(std::pair<uint32_t, uint32_t> base, uint32_t multiplier, uint32_t levels, const std::vector<int>& devices,
                uint32_t frames_in_flight = 1, uint32_t frames_per_batch = 1) {
        std::memset(&cfg_, 0, sizeof cfg_);
        check(bhray_ladder_from_base(base.first, base.second, multiplier, levels, &cfg_));
        if (devices.empty() || devices.size() > BHRAY_MAX_DEVICES) throw std::runtime_error("bhray: bad device list");
        cfg_.device_count = (uint32_t)devices.size();
        for (size_t i = 0; i < devices.size(); i++) cfg_.devices[i] = devices[i];
        cfg_.frames_in_flight = frames_in_flight; cfg_.frames_per_batch = frames_per_batch;
        check(bhray_create(&cfg_, &ctx_));
    }
    // The reference host's own configuration: the shipped 72x41 x3 x4 ladder, `frames_in_flight` = the swap chain's
    // desired_maximum_frame_latency (2, mod.rs:108), optionally BHRAY_F_TEMPORAL (consecutive frames of an interactive host are similar)
    RayPipeline(std::pair<uint32_t, uint32_t> base, uint32_t multiplier, uint32_t levels, int device, uint32_t frames_in_flight, uint32_t flags,
                uint32_t speculative_levels) {
        std::memset(&cfg_, 0, sizeof cfg_);
        check(bhray_ladder_from_base(base.first, base.second, multiplier, levels, &cfg_));
        cfg_.device = device; cfg_.frames_in_flight = frames_in_flight; cfg_.flags = flags; cfg_.speculative_levels = speculative_levels;
        check(bhray_create(&cfg_, &ctx_));
    }
    RayPipeline(const RayPipeline&) = delete;
    ~RayPipeline() {
        if (ctx_) (void)bhray_sync(ctx_);
        for (void* p : staging_) (void)bhray_host_free(p);
        bhray_destroy(ctx_);
    }
    // ---- the drop-in shim's per-frame pair: pass_handoff() where the reference dispatches its ray pipelines
    // (mod.rs:415-417), finish() where the host needs the pixels (before sky_pipeline.pass(), mod.rs:419)
    void enable_handoff(Handoff h, uint32_t frames_in_flight) {
        handoff_ = h; ring_ = frames_in_flight < 1 ? 1 : frames_in_flight;
        const size_t bytes = (size_t)cfg_.frame_w * cfg_.frame_h * (h == Handoff::AsyncDisplay ? 4 : (h == Handoff::AsyncSky ? 8 : 16));
        for (uint32_t i = 0; i < ring_; i++) { void* p = nullptr; check(bhray_host_alloc(bytes, &p)); staging_.push_back(p); }
        tickets_.assign(ring_, 0); pending_.assign(ring_, false);
    }
    void pass_handoff() {
        const uint32_t k = (uint32_t)(frame_ % ring_);
        if (pending_[k]) { check(bhray_wait_read(ctx_, tickets_[k]), ctx_); pending_[k] = false; }   // (finish() already took it unless the host skipped a frame)
        pass();
        if (handoff_ == Handoff::AsyncHdr) {
            check(bhray_read_hdr_async(ctx_, (float*)staging_[k], (size_t)cfg_.frame_w * 16, &tickets_[k]), ctx_); pending_[k] = true;
        } else if (handoff_ == Handoff::AsyncSky) {
            resolve_sky();
            check(bhray_read_sky_async(ctx_, (uint16_t*)staging_[k], (size_t)cfg_.frame_w * 8, &tickets_[k]), ctx_); pending_[k] = true;
        } else if (handoff_ == Handoff::AsyncDisplay) {
            resolve_display();
            check(bhray_read_display_async(ctx_, (uint8_t*)staging_[k], (size_t)cfg_.frame_w * 4, &tickets_[k]), ctx_); pending_[k] = true;
        }
        frame_++;
    }
    // The pixels the host uploads into its texture (queue.write_texture): Sync - the frame just rendered (RGBA32F); Async* - the OLDEST
    // frame in flight, i.e. the frame enqueued ring-1 passes ago (nullptr while the pipeline fills): with a ring of 2 the host shows frame
    // k-1 while frame k renders, which is what its swap chain's frame latency of 2 does to every frame anyway.
    const void* finish() {
        if (handoff_ == Handoff::Sync) {
            check(bhray_read_hdr(ctx_, (float*)staging_[0], (size_t)cfg_.frame_w * 16), ctx_);
            return staging_[0];
        }
        if (frame_ < ring_) return nullptr;
        const uint32_t k = (uint32_t)(frame_ % ring_);             // the slot the NEXT pass reuses = the oldest frame in flight
        if (pending_[k]) { check(bhray_wait_read(ctx_, tickets_[k]), ctx_); pending_[k] = false; }
        return staging_[k];
    }
    // after the last pass: the k-th oldest frame still in flight (k = 1 .. ring-1), already drained - what the next finish() calls would hand over
    const void* finish_pending(uint32_t k) {
        if (handoff_ == Handoff::Sync || frame_ < k || k >= ring_) return nullptr;
        return staging_[(size_t)((frame_ + k) % ring_)];
    }
    void drain() { for (uint32_t k = 0; k < ring_; k++) if (pending_.size() > k && pending_[k]) { check(bhray_wait_read(ctx_, tickets_[k]), ctx_); pending_[k] = false; } }
    std::pair<uint32_t, uint32_t> resolution() const { return {cfg_.frame_w, cfg_.frame_h}; }
    void set_texture(int slot, const uint8_t* rgba8, uint32_t w, uint32_t h) { check(bhray_set_texture(ctx_, slot, rgba8, w, h), ctx_); }
    void upload_model(const Model& m, uint32_t index = 0) { bhray_model_desc d = m.desc(); check(bhray_upload_model(ctx_, index, &d), ctx_); }
    // the tree built on the GPU from the model's points, normals and triangles; update_model_vertices then moves them without a host build
    void upload_model_build(const Model& m, uint32_t index = 0) { bhray_model_desc d = m.desc(); check(bhray_upload_model_build(ctx_, index, &d), ctx_); }
    void update_model_vertices(uint32_t index, const float* points, int32_t point_count, const float* normals, int32_t normal_count) {
        check(bhray_update_model_vertices(ctx_, index, points, point_count, normals, normal_count), ctx_);
    }
    // affine pose of a device-built slot, applied on the GPU (row-major 3x4, bhray_pose_from_euler makes one; nullptr: the rest geometry)
    void set_model_pose(uint32_t index, const float* pose_3x4) { check(bhray_set_model_pose(ctx_, index, pose_3x4), ctx_); }
    void set_model_transform(uint32_t index, const float position[3], int32_t visible) { check(bhray_set_model_transform(ctx_, index, position, visible), ctx_); }
    void set_mesh_lensing(bool on) { check(bhray_set_mesh_lensing(ctx_, on ? 1 : 0), ctx_); }   // lensed meshes: from the next pass on
    void set_mesh_lensing_word(int32_t on) { check(bhray_set_mesh_lensing(ctx_, on), ctx_); }    // ... the setting's whole word: BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS lenses the ray batches too
    void set_materials(const void* material_uniforms_128) { check(bhray_set_materials(ctx_, material_uniforms_128, 128), ctx_); }   // mod.rs:389 (ignored by the shader)
    void set_uniforms(const bhray_camera_uniform& c, const bhray_black_hole_uniform& b, const bhray_details& d) { check(bhray_set_uniforms(ctx_, &c, &b, &d), ctx_); }
    void pass() { check(bhray_render(ctx_), ctx_); }                                            // ray_pipeline.rs:301-309
    void flush() { check(bhray_flush(ctx_), ctx_); }
    void set_sky_filter(bool on) { check(bhray_set_sky_filter(ctx_, on ? 1 : 0), ctx_); }        // footprint-filtered sky pass: from the next resolve_sky / resolve_display on
    // point stars: a catalogue lensed into the sky pass from the next resolve_sky / resolve_display on; an empty vector removes it
    void set_stars(const std::vector<bhray_star>& stars, const bhray_star_params* params = nullptr) {
        check(bhray_set_stars(ctx_, stars.empty() ? nullptr : stars.data(), (uint32_t)stars.size(), params), ctx_);
    }
    void resolve_sky() { check(bhray_resolve_sky(ctx_), ctx_); }                                // sky_pipeline.rs pass
    // bloom / mix / hdr / fxaa passes (mod.rs:425-431), with the uniforms Renderer::render uploads unless set_post_uniforms changed them
    void resolve_display() { check(bhray_resolve_display(ctx_), ctx_); }
    void set_post_uniforms(const bhray_fxaa_details& f, const bhray_mix_details& m) { check(bhray_set_post_uniforms(ctx_, &f, &m), ctx_); }
    std::vector<float> output() {                                                               // output_view + read-back
        std::vector<float> out((size_t)cfg_.frame_w * cfg_.frame_h * 4);
        check(bhray_read_hdr(ctx_, out.data(), (size_t)cfg_.frame_w * 16), ctx_);
        return out;
    }
    // ray batches (bhray_trace_rays): what trace_ray returns for each ray under the current uniforms, textures and models - 4 f32 per ray
    std::vector<float> trace_rays(const std::vector<bhray_ray>& rays) {
        std::vector<float> out(rays.size() * 4);
        check(bhray_trace_rays(ctx_, rays.data(), (uint32_t)rays.size(), out.data()), ctx_);
        return out;
    }
    // ray records (bhray_trace_rays_records): trace_rays, and per ray its first hit, the model and triangle, where, the iterations, the closest approach and
    // the light left; `results` (4 f32 per ray) is filled when it is not null
    std::vector<bhray_ray_record> trace_rays_records(const std::vector<bhray_ray>& rays, std::vector<float>* results = nullptr) {
        std::vector<bhray_ray_record> records(rays.size());
        if (results) results->assign(rays.size() * 4, 0.0f);
        check(bhray_trace_rays_records(ctx_, rays.data(), (uint32_t)rays.size(), results ? results->data() : nullptr, records.data()), ctx_);
        return records;
    }
    // ray paths (bhray_trace_rays_paths): trace_rays_records, and per ray the sampled curve the integrator walked - ray r's points at
    // points[r * max_points + k], k < min(counts[r], max_points); counts[r] = (iterations >> stride_log2) + 2 whatever max_points is
    struct RayPaths { std::vector<bhray_ray_record> records; std::vector<bhray_path_point> points; std::vector<uint32_t> counts; uint32_t max_points; };
    RayPaths trace_rays_paths(const std::vector<bhray_ray>& rays, uint32_t stride_log2, uint32_t max_points, std::vector<float>* results = nullptr) {
        RayPaths p;
        p.max_points = max_points;
        p.records.resize(rays.size());
        p.points.resize(rays.size() * (size_t)max_points);
        p.counts.resize(rays.size());
        if (results) results->assign(rays.size() * 4, 0.0f);
        check(bhray_trace_rays_paths(ctx_, rays.data(), (uint32_t)rays.size(), stride_log2, max_points, results ? results->data() : nullptr, p.records.data(),
                                     p.points.data(), p.counts.data()), ctx_);
        return p;
    }
    // supersampled stills (bhray_accum_*): the accumulation image cleared, `samples` jittered samples per frame pixel added under the current uniforms,
    // and their mean - RGBA32F, sky resolved, 4 f32 per pixel.  Sample 0 is the pixel centre.
    std::vector<float> accumulate(uint32_t samples) {
        check(bhray_accum_begin(ctx_), ctx_);
        check(bhray_accum_add(ctx_, samples), ctx_);
        std::vector<float> out((size_t)cfg_.frame_w * cfg_.frame_h * 4);
        check(bhray_accum_read(ctx_, out.data(), (size_t)cfg_.frame_w * 16), ctx_);
        return out;
    }
    // adaptive stills (bhray_accum_add_adaptive): the accumulation image cleared, every pixel sampled until the error of its mean is under the bound
    // or it has max_samples, and the mean as accumulate() delivers it.  info (may be null): what the call did; counts (may be null): the samples issued per pixel.
    std::vector<float> accumulate_adaptive(const bhray_accum_adaptive& params, bhray_accum_adaptive_info* info = nullptr, std::vector<uint32_t>* counts = nullptr) {
        check(bhray_accum_begin(ctx_), ctx_);
        check(bhray_accum_add_adaptive(ctx_, &params, info), ctx_);
        std::vector<float> out((size_t)cfg_.frame_w * cfg_.frame_h * 4);
        check(bhray_accum_read(ctx_, out.data(), (size_t)cfg_.frame_w * 16), ctx_);
        if (counts) {
            counts->resize((size_t)cfg_.frame_w * cfg_.frame_h);
            check(bhray_accum_read_counts(ctx_, counts->data(), (size_t)cfg_.frame_w * 4), ctx_);
        }
        return out;
    }
    // still cameras (bhray_accum_set_camera): the camera model of accumulate() / accumulate_adaptive() from the next call on; null: pinhole, no lens.
    // struct_size is filled in here.
    void set_still_camera(const bhray_still_camera* camera) {
        if (!camera) { check(bhray_accum_set_camera(ctx_, nullptr), ctx_); return; }
        bhray_still_camera c = *camera;
        c.struct_size = (uint32_t)sizeof(bhray_still_camera);
        check(bhray_accum_set_camera(ctx_, &c), ctx_);
    }
    // still pixel filters (bhray_accum_set_filter): the reconstruction filter of accumulate() from the next call on; null: the box.
    // struct_size is filled in here.  accumulate_adaptive() is refused under a filter other than the box.
    void set_still_filter(const bhray_still_filter* filter) {
        if (!filter) { check(bhray_accum_set_filter(ctx_, nullptr), ctx_); return; }
        bhray_still_filter f = *filter;
        f.struct_size = (uint32_t)sizeof(bhray_still_filter);
        check(bhray_accum_set_filter(ctx_, &f), ctx_);
    }
    // point stars in stills (bhray_accum_set_stars): with on and a catalogue in force (set_stars), every sample image of accumulate() receives the
    // catalogue's stars before it is summed, from the next call on.  accumulate() under a lens and accumulate_adaptive() are then refused.
    void set_still_stars(bool on) { check(bhray_accum_set_stars(ctx_, on ? 1 : 0), ctx_); }
    // the moving observer of a still (bhray_accum_set_observer): every look direction of accumulate() / accumulate_adaptive() aberrated by the velocity
    // (static frame, world axes, units of c) and, with beaming, every sample scaled by D^4, from the next call on; a zero velocity: at rest.  struct_size is filled in here.
    void set_still_observer(bhray_observer observer) {
        observer.struct_size = (uint32_t)sizeof(bhray_observer);
        check(bhray_accum_set_observer(ctx_, &observer), ctx_);
    }
    // still passes (bhray_accum_set_passes): the per-pixel maps the NEXT accumulate() carries beside its colour - an OR of BHRAY_PASS_*; 0: none.
    // accumulate_adaptive() is refused in an accumulation that carries passes.
    void set_still_passes(uint32_t passes) { check(bhray_accum_set_passes(ctx_, passes), ctx_); }
    // one pass of the current accumulation (bhray_accum_read_pass): the mean over its samples under its filter, RGBA32F, 4 f32 per pixel
    std::vector<float> still_pass(uint32_t pass) {
        std::vector<float> out((size_t)cfg_.frame_w * cfg_.frame_h * 4);
        check(bhray_accum_read_pass(ctx_, pass, out.data(), (size_t)cfg_.frame_w * 16), ctx_);
        return out;
    }
    // denoised stills (bhray_accum_read_denoised): the current accumulation's image through the a-trous filter guided by its passes, RGBA32F;
    // null: the library's defaults.  struct_size is filled in here.  The accumulation must carry passes (set_still_passes) and must not be adaptive.
    std::vector<float> accumulation_denoised(const bhray_still_denoise* denoise = nullptr) {
        std::vector<float> out((size_t)cfg_.frame_w * cfg_.frame_h * 4);
        if (!denoise) { check(bhray_accum_read_denoised(ctx_, nullptr, out.data(), (size_t)cfg_.frame_w * 16), ctx_); return out; }
        bhray_still_denoise d = *denoise;
        d.struct_size = (uint32_t)sizeof(bhray_still_denoise);
        check(bhray_accum_read_denoised(ctx_, &d, out.data(), (size_t)cfg_.frame_w * 16), ctx_);
        return out;
    }
    bhray_ctx* ctx() { return ctx_; }
private:
    bhray_config cfg_;
    bhray_ctx* ctx_ = nullptr;
    Handoff handoff_ = Handoff::Sync;
    uint32_t ring_ = 1;
    uint64_t frame_ = 0;
    std::vector<void*> staging_;
    std::vector<uint64_t> tickets_;
    std::vector<bool> pending_;
};

// A 360 x 180 degree panorama's rays (bhusie_amd/cameras.py: equirect_rays): pixel centres, column i at longitude (i - (w - 1) / 2) * 2 pi / w from `forward` towards
// `right`, row j at latitude (j - (h - 1) / 2) * pi / h towards `up`, in create_ray's basis (plane_up = (0, -1, 0): ray.wgsl:275-277); binary32 throughout, directions
// normalised as the kernels expect (v * (1 / sqrt(dot(v, v)))).
inline std::vector<bhray_ray> equirect_rays(const float position[3], const float forward[3], uint32_t w, uint32_t h) {
    auto cross = [](const float a[3], const float b[3], float o[3]) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
    auto normalize = [](float v[3]) { const float r = 1.0f / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); v[0] *= r; v[1] *= r; v[2] *= r; };
    const float plane_up[3] = {0.0f, -1.0f, 0.0f};
    float fwd[3] = {forward[0], forward[1], forward[2]}, right[3], up[3];
    cross(fwd, plane_up, right); normalize(right);
    cross(fwd, right, up); normalize(up);
    normalize(fwd);
    const float pi = 3.14159274f;
    std::vector<bhray_ray> rays((size_t)w * h);
    for (uint32_t j = 0; j < h; j++) {
        const float lat = ((float)j - (float)(h - 1) * 0.5f) * (pi / (float)h);
        const float cp = std::cos(lat), sp = std::sin(lat);
        for (uint32_t i = 0; i < w; i++) {
            const float lon = ((float)i - (float)(w - 1) * 0.5f) * (2.0f * pi / (float)w);
            const float a = cp * std::cos(lon), b = cp * std::sin(lon);
            bhray_ray& r = rays[(size_t)j * w + i];
            float d[3];
            for (int k = 0; k < 3; k++) d[k] = (fwd[k] * a + right[k] * b) + up[k] * sp;
            normalize(d);
            for (int k = 0; k < 3; k++) { r.origin[k] = position[k]; r.direction[k] = d[k]; }
            r.pad0 = 0.0f; r.pad1 = 0.0f;
        }
    }
    return rays;
}

// create_ray (ray.wgsl:269-285) for pixel (x, y) of a w x h level, as bhusie_amd/cameras.py: pinhole_rays forms it - binary32, operation by operation, tan(fov / 2) as the
// library's portable sine over cosine (bhray_math.h: bh_sincos, restated here because this header sees the C ABI only).  Build without floating-point contraction.
namespace detail {
inline float sincos_portable(float xin, int kind) {          // kind 0: sin, 1: cos
    float x = std::fabs(xin);
    bool sign = kind == 0 ? std::signbit(xin) : false;
    if (!(x <= 3.0e9f)) return std::nanf("");
    uint32_t j = (uint32_t)(x * 1.27323954f);
    j = j + (j & 1u);
    const float y = (float)j;
    x = ((x - y * 0.78515625f) - y * 2.4187564849853515625e-4f) - y * 3.77489497744594108e-8f;
    j = j & 7u;
    if (j > 3u) { sign = !sign; j = j - 4u; }
    if (kind == 1 && j > 1u) sign = !sign;
    const float z = x * x;
    const bool mid = (j == 1u || j == 2u);
    const bool use_cos = kind == 0 ? mid : !mid;
    float r;
    if (use_cos) {
        float p = 2.443315711809948e-5f;
        p = p * z - 1.388731625493765e-3f;
        p = p * z + 4.166664568298827e-2f;
        r = ((p * z) * z - 0.5f * z) + 1.0f;
    } else {
        float p = -1.9515295891e-4f;
        p = p * z + 8.3321608736e-3f;
        p = p * z - 1.6666654611e-1f;
        r = (p * z) * x + x;
    }
    return sign ? -r : r;
}
}  // namespace detail
inline bhray_ray pinhole_ray(const float position[3], const float forward[3], float fov, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
    auto cross = [](const float a[3], const float b[3], float o[3]) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
    auto normalize = [](float v[3]) { const float r = 1.0f / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); v[0] *= r; v[1] *= r; v[2] *= r; };
    const float plane_up[3] = {0.0f, -1.0f, 0.0f};
    float right[3], up[3];
    cross(forward, plane_up, right); normalize(right);
    cross(forward, right, up); normalize(up);
    const uint32_t sm = (w - 1) < (h - 1) ? (w - 1) : (h - 1);
    const float increment = 1.0f / (float)sm;
    const float posx = (2.0f * ((float)x - (float)(w - 1) * 0.5f)) * increment;
    const float posy = (2.0f * ((float)y - (float)(h - 1) * 0.5f)) * increment;
    const float half = fov / 2.0f;
    const float fov_factor = 1.0f / (detail::sincos_portable(half, 0) / detail::sincos_portable(half, 1));
    bhray_ray r;
    float d[3];
    for (int k = 0; k < 3; k++) d[k] = (right[k] * posx + up[k] * posy) + forward[k] * fov_factor;
    normalize(d);
    for (int k = 0; k < 3; k++) { r.origin[k] = position[k]; r.direction[k] = d[k]; }
    r.pad0 = 0.0f; r.pad1 = 0.0f;
    return r;
}

// Renderer::{new, render} restricted to the ray pass.
class Renderer {
public:
    Camera camera;
    BlackHole black_hole;
    RayDetails ray_details;
    bool mesh_lensing = false;      // lensed meshes (bhray_set_mesh_lensing): models are tested inside the relativity sphere too; applied before each render
    bhray_observer observer{(uint32_t)sizeof(bhray_observer), {0.0f, 0.0f, 0.0f}, 1u};   // the moving observer of the stills; zero velocity: at rest; applied before each still
    uint32_t still_passes = 0;      // still passes: the BHRAY_PASS_* maps render_still carries beside its colour (still_pass reads them); applied before each still
    bool lens_ray_batches = false;  // ... and, with it, in ray batches too (BHRAY_LENS_RAYS): render_rays, pick and the stills trace lensed; ray_path throws the ctx's error
    explicit Renderer(int device = 0) : ray_pipeline_({72, 41}, 3, 4, device) {}               // mod.rs:177-179
    Renderer(std::pair<uint32_t, uint32_t> base, uint32_t multiplier, uint32_t levels, int device = 0) : ray_pipeline_(base, multiplier, levels, device) {}
    Renderer(std::pair<uint32_t, uint32_t> base, uint32_t multiplier, uint32_t levels, const std::vector<int>& devices) : ray_pipeline_(base, multiplier, levels, devices) {}
    // the drop-in host: frames_in_flight = the swap chain's frame latency, a hand-off form, optionally temporal speculation
    Renderer(std::pair<uint32_t, uint32_t> base, uint32_t multiplier, uint32_t levels, int device, uint32_t frames_in_flight, Handoff h, bool temporal)
        : ray_pipeline_(base, multiplier, levels, device, frames_in_flight, temporal ? (uint32_t)BHRAY_F_TEMPORAL : 0u, temporal ? 0u : (levels >= 4 ? 3u : (levels >= 3 ? 2u : 0u))) {       // a host that shows every frame wants the shortest chain: 3 speculative levels (1.08 against 1.21 ms with 2)
        ray_pipeline_.enable_handoff(h, frames_in_flight);
    }
    RayPipeline& ray_pipeline() { return ray_pipeline_; }
    // scene.models: slot i holds the i-th model; model_count = how many (mod.rs:384).  set_model replaces slot 0, add_model takes the next
    // slot and returns its index (BHRAY_MAX_MODELS slots).
    void set_model(const Model& m) { ray_pipeline_.upload_model(m, 0); if (models_ == 0) models_ = 1; ray_details.model_count = (int32_t)models_; }
    uint32_t add_model(const Model& m, bool build_on_device = false) {
        if (models_ >= BHRAY_MAX_MODELS) throw std::runtime_error("add_model: the ctx holds BHRAY_MAX_MODELS models");
        if (build_on_device) ray_pipeline_.upload_model_build(m, models_);
        else ray_pipeline_.upload_model(m, models_);
        ray_details.model_count = (int32_t)++models_;
        return models_ - 1;
    }
    void render(float dt) {                                                                     // mod.rs:378-420
        ray_details.time += dt;                                                                 // mod.rs:382
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);        // mod.rs:386-388
        const float materials[32] = {0};
        ray_pipeline_.set_materials(materials);                                                 // mod.rs:389
        apply_lensing();
        ray_pipeline_.pass();
    }
    // the same frame through the drop-in shim: update + pass_handoff (mod.rs:378-417), then finish() where the sky pass would start
    const void* render_handoff(float dt) {
        ray_details.time += dt;
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);
        const float materials[32] = {0};
        ray_pipeline_.set_materials(materials);
        apply_lensing();
        ray_pipeline_.pass_handoff();
        return ray_pipeline_.finish();
    }
    // an image through caller-supplied rays (w * h of them, row 0 the top) under this renderer's black hole, details, textures and models: RGBA32F as output()
    std::vector<float> render_rays(const std::vector<bhray_ray>& rays) {
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);
        apply_lensing();
        return ray_pipeline_.trace_rays(rays);
    }
    // a supersampled still of the current scene: the mean of `samples` jittered samples per frame pixel (RayPipeline::accumulate), RGBA32F as output() after the sky pass
    // still_camera (may be null: the pinhole): the still as a panorama, a fisheye or through a thin lens from the camera's position along its forward
    // (RayPipeline::set_still_camera)
    // still_filter (may be null: the box): the pixel reconstruction filter, a tent or a Mitchell-Netravali cubic (RayPipeline::set_still_filter)
    std::vector<float> render_still(uint32_t samples, const bhray_still_camera* still_camera = nullptr) { return render_still(samples, still_camera, nullptr); }
    // stars: the catalogue of RayPipeline::set_stars lensed into every sample's image (RayPipeline::set_still_stars)
    std::vector<float> render_still(uint32_t samples, const bhray_still_camera* still_camera, const bhray_still_filter* still_filter, bool stars = false) {
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);
        apply_lensing();
        ray_pipeline_.set_still_camera(still_camera);
        ray_pipeline_.set_still_filter(still_filter);
        ray_pipeline_.set_still_stars(stars);
        ray_pipeline_.set_still_observer(observer);
        ray_pipeline_.set_still_passes(still_passes);
        return ray_pipeline_.accumulate(samples);
    }
    // the last render_still denoised (RayPipeline::accumulation_denoised): that still must have carried passes (still_passes != 0).  Reads only: the
    // plain still, its passes and further denoised reads with other parameters stay available.
    std::vector<float> still_denoised(const bhray_still_denoise* denoise = nullptr) { return ray_pipeline_.accumulation_denoised(denoise); }
    // one pass of the last render_still (still_passes; RayPipeline::still_pass): BHRAY_PASS_COVERAGE, _GEOMETRY, _POSITION or _ESCAPE
    std::vector<float> still_pass(uint32_t pass) { return ray_pipeline_.still_pass(pass); }
    // an adaptive still of the current scene (RayPipeline::accumulate_adaptive): params.struct_size is filled in here
    std::vector<float> render_still_adaptive(bhray_accum_adaptive params, bhray_accum_adaptive_info* info = nullptr, std::vector<uint32_t>* counts = nullptr,
                                             const bhray_still_camera* still_camera = nullptr) {
        params.struct_size = (uint32_t)sizeof(bhray_accum_adaptive);
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);
        apply_lensing();
        ray_pipeline_.set_still_camera(still_camera);
        ray_pipeline_.set_still_filter(nullptr);                  // an adaptive still has no filter but the box
        ray_pipeline_.set_still_stars(false);                     // and no point stars
        ray_pipeline_.set_still_observer(observer);
        ray_pipeline_.set_still_passes(0);                        // and no passes
        return ray_pipeline_.accumulate_adaptive(params, info, counts);
    }
    // what is under frame pixel (x, y): the record of that pixel's pinhole ray under the current scene (hit & 0xff: BHRAY_HIT_*; (hit >> 8) & 0xff: the model slot of a mesh hit)
    bhray_ray_record pick(uint32_t x, uint32_t y) {
        const auto res = ray_pipeline_.resolution();
        if (x >= res.first || y >= res.second) throw std::runtime_error("bhray: pick: the pixel lies outside the frame");
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);
        apply_lensing();
        return ray_pipeline_.trace_rays_records({pinhole_ray(camera.position, camera.forward, camera.fov, res.first, res.second, x, y)})[0];
    }
    // the light path behind frame pixel (x, y): pick's record, and the points of that pixel's pinhole ray from the camera to where trace_ray's loop ended - one per
    // 2^stride_log2 iterations and the end point; the row is sized from max_iterations, so nothing is dropped
    struct RayPath { bhray_ray_record record; std::vector<bhray_path_point> points; };
    RayPath ray_path(uint32_t x, uint32_t y, uint32_t stride_log2 = 0) {
        const auto res = ray_pipeline_.resolution();
        if (x >= res.first || y >= res.second) throw std::runtime_error("bhray: ray_path: the pixel lies outside the frame");
        if (stride_log2 > BHRAY_MAX_PATH_STRIDE_LOG2) throw std::runtime_error("bhray: ray_path: the stride's logarithm is at most 16");
        ray_pipeline_.set_uniforms(camera.uniform(), black_hole.uniform(), ray_details);
        apply_lensing();
        const uint32_t max_points = ((uint32_t)ray_details.max_iterations >> stride_log2) + 2u;
        auto p = ray_pipeline_.trace_rays_paths({pinhole_ray(camera.position, camera.forward, camera.fov, res.first, res.second, x, y)}, stride_log2, max_points);
        RayPath out;
        out.record = p.records[0];
        out.points.assign(p.points.begin(), p.points.begin() + (p.counts[0] < max_points ? p.counts[0] : max_points));
        return out;
    }
private:
    // the ctx is told BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS, BHRAY_LENS_FRAMES or 0; compared is the word last sent, not its truth (1 and 3 are different settings)
    void apply_lensing() {
        const int32_t word = mesh_lensing ? (lens_ray_batches ? (BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS) : BHRAY_LENS_FRAMES) : 0;
        if (word != lensing_applied_) { ray_pipeline_.set_mesh_lensing_word(word); lensing_applied_ = word; }
    }
    RayPipeline ray_pipeline_;
    uint32_t models_ = 0;
    int32_t lensing_applied_ = 0;   // the word the ctx was last told (its default: off)
};

}  // namespace bhusie
