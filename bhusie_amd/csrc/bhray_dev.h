// bhray_dev.h — the per-device engine behind the public bhray_ctx.
//
// A bhray_dev renders ONE row partition of the frame on ONE GPU (bhray_api.hip): ladder levels, frame slots, frame batches,
// speculative levels.  The public bhray_ctx (bhray_group.hip) owns one bhray_dev per local partition and, when the frame is
// split over several partitions, the gather of the row tiles to the root partition's GPU (RCCL) and the de-interleave into
// the frame.  Nothing here is exported; the C ABI is include/bhray.h (and include/bhray_diag.h for measurement).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/bhray_diag.h"

#include <vector>

struct bhray_dev;

namespace bhray {
// Row partition arithmetic shared by the engine, the gather tables and the ABI helpers (bhray_config.partition).
// nullptr: the partition described by cfg for `world` partitions is valid; otherwise what is wrong with it.
inline const char* partition_error(const bhray_config& cfg, uint32_t world) {
    if (world < 1) return "no partitions";
    if (cfg.partition == BHRAY_PARTITION_STRIPES) return cfg.stripe_rows < 1 ? "stripe_rows must be >= 1" : nullptr;
    if (cfg.partition != BHRAY_PARTITION_SLABS) return "unknown partition mode";
    if (world > BHRAY_MAX_DEVICES) return "BHRAY_PARTITION_SLABS: more partitions than slab_row0 holds";
    if (cfg.slab_row0[0] != 0 || cfg.slab_row0[world] != cfg.frame_h) return "BHRAY_PARTITION_SLABS: slab_row0 must start at 0 and end at frame_h";
    for (uint32_t p = 0; p < world; p++) if (cfg.slab_row0[p] > cfg.slab_row0[p + 1]) return "BHRAY_PARTITION_SLABS: slab_row0 must be non-decreasing";
    return nullptr;
}
// frame rows of partition `part`, increasing (a valid partition: partition_error)
inline std::vector<uint32_t> partition_row_list(const bhray_config& cfg, uint32_t world, uint32_t part) {
    std::vector<uint32_t> rows;
    if (cfg.partition == BHRAY_PARTITION_SLABS) {
        for (uint32_t r = cfg.slab_row0[part]; r < cfg.slab_row0[part + 1]; r++) rows.push_back(r);
    } else {
        for (uint32_t r = 0; r < cfg.frame_h; r++) if ((r / cfg.stripe_rows) % world == part) rows.push_back(r);
    }
    return rows;
}
// rows of level k-1 that the rows `fine` (sorted) of level k read (ray.wgsl:185-201), same binary32 arithmetic as the kernels' (bhray_api.hip)
std::vector<int32_t> coarse_rows_needed(const std::vector<int32_t>& fine, int h, int ph);

struct DevOptions {
    bool external_out = false;   // the ctx binds every frame's destination (send buffer / assembled frame): no own output buffers
    bool frame_rowmap = false;   // the destination is a whole frame_h x frame_w frame: row r of the frame lands in row r (root partition of a gather)
    uint32_t max_streams = 0;    // > 0: at most this many HIP streams for the frame slots (the slots beyond share them) - several engines on ONE physical GPU
                                 // (functional tests of the multi-GPU path on a one-GPU box) must stay within the device's hardware queues TOGETHER
};

// The three images of the most recently staged frame that a ctx hands to its host, each by a blocking read, an asynchronous
// read that returns a ticket, and a device pointer.
enum ImageKind { IMAGE_HDR, IMAGE_SKY, IMAGE_DISPLAY };   // RGBA32F ray-pass frame, RGBA16F sky image, RGBA8 display image

// What either layer's last_image() says about one of them: where it lies and on which stream it is produced.  rows == 0: nothing to copy
// here (this partition owns no rows; the frame lives on another rank) - stream is then the stream a ticket's event is recorded on, or NULL.
struct FrameImage {
    const void* src = nullptr;
    size_t row_bytes = 0, rows = 0;    // tightly packed rows
    hipStream_t stream = nullptr;
    bool render_target = false;        // the slot's next render writes into this very buffer: a copy enqueued on `stream` must be ordered ahead of it
    bool fits(const void* dst, size_t pitch) const { return dst && pitch >= row_bytes; }
    // device -> host, one copy for a tight pitch; enqueued on `stream`, or blocking (the caller has synchronised what produces the image)
    hipError_t copy_to(void* dst, size_t pitch, bool async) const {
        if (!async) return hipMemcpy2D(dst, pitch, src, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost);
        if (pitch == row_bytes) return hipMemcpyAsync(dst, src, rows * row_bytes, hipMemcpyDeviceToHost, stream);
        return hipMemcpy2DAsync(dst, pitch, src, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, stream);
    }
};

// Tickets of the asynchronous reads: ticket t owns ring position t % SIZE; the event there is recorded behind t's copy.
struct ReadRing {
    static constexpr uint64_t SIZE = 64;
    hipEvent_t ev[SIZE] = {nullptr};
    uint64_t next = 0;                 // tickets issued so far
    // the event of the next ticket: created on first use, otherwise free once the ticket that held it SIZE copies ago has completed (waited for here).
    // Takes no ticket: an error between here and commit() consumes none.
    hipError_t acquire(hipEvent_t* out) {
        hipEvent_t& e = ev[next % SIZE];
        const hipError_t rc = !e ? hipEventCreateWithFlags(&e, hipEventDisableTiming) : (next >= SIZE ? hipEventSynchronize(e) : hipSuccess);
        *out = e;
        return rc;
    }
    // the ticket exists from here on.  Behind the record of acquire()'s event - or without either: a ticket that has nothing to wait for
    // (a rank that does not hold the frame)
    uint64_t commit() { return next++; }
    bool known(uint64_t ticket) const { return ticket < next; }
    // a known ticket: returns once its copy has completed (one more than SIZE old: its event was waited for when it was recycled; never recorded: at once)
    hipError_t wait(uint64_t ticket) const {
        if (next - ticket > SIZE || !ev[ticket % SIZE]) return hipSuccess;
        return hipEventSynchronize(ev[ticket % SIZE]);
    }
    void destroy() { for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
};
}  // namespace bhray

const char* dev_last_error(const bhray_dev* c);            // c may be NULL: last create error of this thread
void dev_set_create_error(const char* msg);
int  dev_create(const bhray_config* cfg, const bhray::DevOptions& opt, bhray_dev** out);
void dev_destroy(bhray_dev* c);
int  dev_set_texture(bhray_dev* c, int slot, const uint8_t* rgba8, uint32_t w, uint32_t h);
int  dev_upload_model_uniform(bhray_dev* c, uint32_t model_index, const void* bytes, size_t size);
int  dev_upload_model(bhray_dev* c, uint32_t model_index, const bhray_model_desc* desc);
int  dev_upload_model_build(bhray_dev* c, uint32_t model_index, const bhray_model_desc* desc);    // tree built on the device (bhray_bvh.hip)
int  dev_update_model_vertices(bhray_dev* c, uint32_t model_index, const float* points, int32_t point_count, const float* normals, int32_t normal_count);
// the arrays in device memory (any device); copied on the build stream behind `after` (may be NULL: nothing to wait for)
int  dev_update_model_vertices_device(bhray_dev* c, uint32_t model_index, const void* d_points, int32_t point_count, const void* d_normals, int32_t normal_count, hipEvent_t after);
int  dev_set_model_pose(bhray_dev* c, uint32_t model_index, const float* pose_3x4);   // affine pose of a device-built slot; NULL: the rest arrays
int  dev_read_model_vertices(bhray_dev* c, uint32_t model_index, float* points, uint32_t point_cap, float* normals, uint32_t normal_cap, uint32_t* point_count, uint32_t* normal_count);
int  dev_get_model_build_info(bhray_dev* c, uint32_t model_index, bhray_model_build_info* out);
int  dev_read_model_bvh(bhray_dev* c, uint32_t model_index, bhray_node* nodes, uint32_t node_cap, int32_t* lookup, uint32_t lookup_cap, uint32_t* node_count, uint32_t* triangle_count);
int  dev_set_model_transform(bhray_dev* c, uint32_t model_index, const float position[3], int32_t visible);
int  dev_set_uniforms(bhray_dev* c, const void* cam32, const void* bh132, const void* det32);
// ray batches: the host variant returns with `out` complete; the device variant enqueues on the engine's query stream, behind what `s` holds and ahead of what it gets
// records / d_records: NULL, or a bhray_ray_record per ray beside the results (the record kernels)
// paths: NULL, or where the sampled paths go (the path kernels) - host memory for dev_trace_rays, device memory for dev_trace_rays_device
struct bhray_dev_paths { uint32_t stride_log2, max_points; bhray_path_point* points /* n * max_points */; uint32_t* counts /* n */; };
int  dev_trace_rays(bhray_dev* c, const bhray_ray* rays, uint32_t n, float* out_rgba32f, uint16_t* sky_rgba16f /* NULL: no sky pass over the results */, bhray_ray_record* records = nullptr,
                    const bhray_dev_paths* paths = nullptr);
int  dev_trace_rays_device(bhray_dev* c, const void* d_rays, uint32_t n, void* d_out_rgba32f, void* d_records, hipStream_t s, const bhray_dev_paths* paths = nullptr);
// the accumulation image: sub-pixel samples of every frame pixel generated, traced, resolved and summed on the query stream; begin clears, add enqueues
// the next sample indices under the current uniforms, the reads wait.  fxaa / mix: the ctx's display uniforms
int  dev_accum_begin(bhray_dev* c);
int  dev_accum_add(bhray_dev* c, uint32_t samples);
int  dev_accum_samples(const bhray_dev* c, uint32_t* total);
int  dev_accum_read(bhray_dev* c, float* dst_rgba32f, size_t pitch);
int  dev_accum_read_display(bhray_dev* c, uint8_t* dst_rgba8, size_t pitch, const bhray_fxaa_details* fxaa, const bhray_mix_details* mix);
int  dev_accum_sample_rays(bhray_dev* c, uint32_t s, bhray_ray* out);   // the generated records of sample s: frame_w * frame_h
int  dev_accum_set_launch_rays(bhray_dev* c, uint32_t max_rays);        // rays per trace launch of dev_accum_add; 0: the default
int  dev_accum_set_camera(bhray_dev* c, const bhray_still_camera* cam); // still cameras: validates and stores; NULL: pinhole, no lens
int  dev_accum_set_observer(bhray_dev* c, const bhray_observer* obs);   // the moving observer: validates and stores; NULL: at rest
int  dev_accum_set_filter(bhray_dev* c, const bhray_still_filter* filter); // still pixel filters: validates and stores; NULL: the box
int  dev_accum_set_passes(bhray_dev* c, uint32_t passes);  // still passes: validates and stores; the next dev_accum_begin takes the set
int  dev_accum_passes(const bhray_dev* c, uint32_t* passes);   // the set of the current accumulation; 0 before dev_accum_begin
int  dev_accum_read_pass(bhray_dev* c, uint32_t pass, float* dst_rgba32f, size_t pitch);   // the mean of one pass's plane, like dev_accum_read
// denoised stills: dev_accum_read / dev_accum_read_display behind the a-trous filter guided by the passes; p == nullptr: the defaults
int  dev_accum_read_denoised(bhray_dev* c, const bhray_still_denoise* p, float* dst_rgba32f, size_t pitch);
int  dev_accum_denoise_times(bhray_dev* c, const bhray_still_denoise* p, float ms[6]);   // bhray_diag.h: its launches' times from events; no image
int  dev_accum_read_display_denoised(bhray_dev* c, const bhray_still_denoise* p, uint8_t* dst_rgba8, size_t pitch, const bhray_fxaa_details* fx, const bhray_mix_details* mx);
int  dev_accum_set_stars(bhray_dev* c, int32_t on);        // point stars in stills: validates and stores; 0 (the default) or 1
// adaptive stills: min_samples for every pixel, then rounds of select - wait for the count - sample the failing pixels, until a selection is empty; blocks
int  dev_accum_add_adaptive(bhray_dev* c, const bhray_accum_adaptive* params, bhray_accum_adaptive_info* info);
int  dev_accum_read_counts(bhray_dev* c, uint32_t* dst, size_t pitch);  // issued per pixel; BHRAY_E_STATE unless the accumulation is adaptive
int  dev_accum_active_pixels(bhray_dev* c, const bhray_accum_adaptive* params, uint32_t* out, uint32_t cap, uint32_t* n);   // one selection, no sampling
int  dev_set_mesh_lensing(bhray_dev* c, int32_t on);       // from the next dev_render; BHRAY_E_STATE for on != 0 on a BHRAY_F_LITERAL / BHRAY_F_EVAL_FMA engine
// another row partition (bhray_config.partition / stripe_rows / slab_row0 / row_rank / row_world) for the same frame; synchronises the engine
int  dev_set_partition(bhray_dev* c, uint32_t partition, uint32_t stripe_rows, const uint32_t* slab_row0, uint32_t row_rank, uint32_t row_world);
int  dev_render(bhray_dev* c);
int  dev_flush(bhray_dev* c);
int  dev_sync(bhray_dev* c);
uint32_t dev_local_rows(const bhray_dev* c);
int  dev_local_row_index(const bhray_dev* c, uint32_t i, uint32_t* frame_row);
// the three images of the most recently staged frame (bhray::ImageKind), each three ways; the sky and display images must have been resolved for that frame
int  dev_read(bhray_dev* c, bhray::ImageKind kind, void* dst, size_t pitch);
int  dev_read_async(bhray_dev* c, bhray::ImageKind kind, void* dst, size_t pitch, uint64_t* ticket);   // in stream order behind what produces the image
int  dev_device_ptr(bhray_dev* c, bhray::ImageKind kind, void** p, size_t* bytes);
int  dev_wait_read(bhray_dev* c, uint64_t ticket);
int  dev_read_level(bhray_dev* c, uint32_t level, float* dst, size_t pitch);
int  dev_bind_output(bhray_dev* c, void* p, size_t bytes);     // destination of the NEXT dev_render only
int  dev_resolve_sky(bhray_dev* c);
int  dev_set_sky_filter(bhray_dev* c, int32_t mode);          // 0: sky.wgsl; 1: the footprint filter from the next dev_resolve_sky; synchronises the engine, builds / frees the pyramid
int  dev_set_stars(bhray_dev* c, const bhray_star* stars, uint32_t n, const bhray_star_params* params);   // point stars from the next dev_resolve_sky; n == 0 / NULL removes; synchronises the engine, uploads the index
int  dev_diag_star_image(bhray_dev* c, const float* frame, uint32_t w, uint32_t h, const uint16_t* sky_in, uint16_t* sky_out);
int  dev_read_sky_pyramid_level(bhray_dev* c, uint32_t level, uint16_t* dst_rgba16f, size_t texels);
int  dev_resolve_display(bhray_dev* c, const bhray_fxaa_details* fxaa, const bhray_mix_details* mix);   // display pass (bhray_post.hip) behind the last frame
int  dev_launch_display(bhray_dev* c, const void* sky, void* scratch, void* dst, const bhray_fxaa_details* fxaa, const bhray_mix_details* mix, hipStream_t stream);
int  dev_wait_event(bhray_dev* c, hipEvent_t ev);             // the next render's launches start after ev (ev is owned by the caller)
int  dev_next_stream(bhray_dev* c, void** s);
int  dev_signal_stream(bhray_dev* c, void* s);
int  dev_selftest(bhray_dev* c, uint64_t mismatches[3]);
int  dev_get_trace_builds(bhray_dev* c, uint64_t launches[2]);   // trace launches enqueued so far with an ORIGIN build / with any other
int  dev_get_level_grids(bhray_dev* c, uint32_t slot, bhray_level_grid_info* out);   // trace grids by queue length: the batch `slot` launched last, and this engine's totals
int  dev_get_level_counters(bhray_dev* c, uint32_t level, bhray_counters* out);
int  dev_add_row_work(bhray_dev* c, uint32_t level, uint64_t* acc, uint32_t n);   // acc[y] += iterations of the last render's rays of level row y
int  dev_get_counters(bhray_dev* c, bhray_counters* out);
int  dev_get_err_skip(bhray_dev* c, uint64_t out[3]);   // the RK error-estimate bound in the counting kernels: wave-steps, wave-steps whose lanes all pass, violations
int  dev_get_timing(bhray_dev* c, bhray_timing* out);
// what the frames still held by the slots cost: integrator steps issued by the trace waves (mean per frame) and pixels visited by the classify launches
int  dev_get_work(bhray_dev* c, double* wave_steps_per_frame, double* classify_pixels_per_frame, uint32_t* frames, int* method);   // method: the integrator of the current uniforms (1 = RK)

// hooks for the gather (bhray_group.hip)
int  dev_device(const bhray_dev* c);
// Position (slot, index in the batch) the next dev_render will stage its frame at.  A staged batch of another kernel variant
// (integrator, mesh) than the current uniforms need is launched first, so the position is final.
int  dev_next_position(bhray_dev* c, int* slot, uint32_t* sub);
// The same state read without side effects: batches launched so far (the staging slot is that number modulo the slots), frames staged
// in that slot and the kernel variant they were staged for.  For the caller's mirror of the staging position (issue threads).
void dev_peek_position(const bhray_dev* c, uint64_t* batch_counter, uint32_t* pending, int* method, int* models);   // models: 0 none, 1 flat space only, 2 lensed
// True when launches were enqueued since the last call; reports the slot and the number of frames of the (last) launched batch.
bool dev_take_launched(bhray_dev* c, int* slot, uint32_t* frames);
int* dev_err_flag(bhray_dev* c);                              // the engine's device-side error word (checked by dev_sync)
hipStream_t dev_slot_stream(bhray_dev* c, int slot);
hipEvent_t  dev_slot_done(bhray_dev* c, int slot);            // recorded behind the slot's last launch
// sky.wgsl over an arbitrary RGBA32F image resident on this device, with this partition's sky texture
int  dev_launch_sky(bhray_dev* c, const void* src_rgba32f, void* dst_rgba16f, size_t npix, hipStream_t stream);
