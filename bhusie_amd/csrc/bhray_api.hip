// bhray_api.hip — the C ABI of include/bhray.h on top of the gfx950 kernels.
//
// Plays the role of RayPipeline::{new,pass,output_view}
// (/root/reference/src/renderer/pipelines/ray_pipeline.rs:36-309) and of the ladder / per-frame
// upload code in Renderer::{new,render} (src/renderer/mod.rs:113-207, 378-420).
// All device memory is owned here; there is no CPU rendering path.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <cmath>
#include <string>
#include <vector>

#include "bhray_accum.h"
#include "bhray_accum_filter.h"
#include "bhray_accum_passes.h"
#include "bhray_accum_denoise.h"
#include "bhray_adapt.h"
#include "bhray_stillcam.h"
#include "bhray_bvh_core.h"
#include "bhray_dev.h"
#include "bhray_internal.h"
#include "bhray_math.h"
#include "bhray_skyfilter.h"
#include "bhray_stars.h"
#include "bhray_accum_stars.h"
#include "bhray_observer.h"

using namespace bhray;

namespace {

// Frame slots run on separate HIP streams; ROCm maps streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues, so 4+ slots
// serialise pairwise unless the HOST raises the limit before the HIP runtime initialises (include/bhray.h, frames in flight).
// The library does not touch the process environment.

thread_local std::string g_create_error;

constexpr int SPAN_MAX = BHRAY_MAX_LEVELS + 2;      // trace launches per batch (per-level, + speculative / predicted)
// Timing events of one batch (one entry of the ring bhray_dev::events), nl = ladder levels: three per level - before its classify, between classify and trace, behind its
// trace (a level without a trace launch of its own records the last two together) -, two around the sky pass, two around the temporal mode's prediction + predicted trace
constexpr int ev_level_begin(uint32_t l) { return (int)(3 * l); }
constexpr int ev_level_classified(uint32_t l) { return (int)(3 * l + 1); }
constexpr int ev_level_traced(uint32_t l) { return (int)(3 * l + 2); }
constexpr int ev_sky_begin(uint32_t nl) { return (int)(3 * nl); }
constexpr int ev_sky_end(uint32_t nl) { return (int)(3 * nl + 1); }
constexpr int ev_predicted_begin(uint32_t nl) { return (int)(3 * nl + 2); }
constexpr int ev_predicted_end(uint32_t nl) { return (int)(3 * nl + 3); }
constexpr size_t events_per_batch(uint32_t nl) { return 3 * (size_t)nl + 4; }

#ifndef BHRAY_ROW_VARIANTS
#define BHRAY_ROW_VARIANTS 9         // orderings of a level's rows kept on the device (centre rows at 0, 1/8, ... 1 of the height); < 2 = ascending only
#endif
struct Level {                      // geometry of one ladder level (shared by all frame slots)
    int w = 0, h = 0;
    std::vector<int32_t> rows;      // rows to compute
    int32_t* d_rows = nullptr;
    int32_t* d_rows_near = nullptr; // BHRAY_ROW_VARIANTS orderings of the same rows, tile rows nearest a centre row first (variant v: centre v / (N-1) of the level's height)
    int32_t* d_rowmap = nullptr;    // final level only
    size_t queue_cap = 0;           // entries the level's queue can need: its rows x its columns
    size_t queue_alloc = 0;         // entries allocated per frame (>= queue_cap; grows when the partition changes: dev_set_partition)
};

// Resources of one frame: level images, work queues and output buffer.
struct FrameRes {
    std::vector<float4*> level_out;     // [levels-1] full-size images of the non-final levels
    std::vector<uint32_t*> queue;       // [levels]
    std::vector<float4*> spec_out;      // speculative mode: traced images of levels 1..S-1 (level 0 traces straight into level_out[0])
    uint32_t* spec_queue = nullptr;     // speculative mode: merged, level-tagged queue of levels 0..S-1
    uint32_t* super_queue = nullptr;    // superset speculation: merged, level-tagged queue of the last U levels
    // temporal speculation (BHRAY_F_TEMPORAL): the pixels the previous frame held here had to trace, all levels, level-tagged
    uint32_t* pred_queue = nullptr;     // the predicted launch's queue: built by predict_kernel from the previous frame's marks
    uint32_t* pred_ctl = nullptr;       // [0] entries [1] entries taken: the control words of level BHRAY_MAX_LEVELS-1 in d_qctl (temporal mode has <= 4 levels), reset with them
    std::vector<uint8_t*> need;         // per level: need[y * w + x] = the last exact classification had to trace that pixel
    std::vector<uint32_t*> stamp;       // per level: stamp[y * w + x] == stamp_value <=> the predicted launch traced that pixel this frame
    uint32_t stamp_value = 0;

    uint32_t* d_qctl = nullptr;         // [BHRAY_QCTL_WORDS]: qcount[l], qhead[l], then the work counters   (a slice of Slot::d_qctl)
    unsigned long long* d_work = nullptr;   // [BHRAY_WORK_WORDS] inside that slice: integrator steps the trace waves issued for the frame held here (FrameLaunch::work)
    Counters64* d_counters = nullptr;   // [BHRAY_MAX_LEVELS]                         (a slice of Slot::d_counters)
    unsigned long long* d_row_work = nullptr;   // BHRAY_F_COUNTERS: iterations per level row, level l at bhray_dev::row_work_off[l] (bhray_get_row_work)
    float4* own_out = nullptr;
    float4* out = nullptr;              // where this frame is written (own_out or a bound buffer)
    uint2* sky_out = nullptr;           // RGBA16F image of the sky resolve pass (allocated on first use)
    uint64_t sky_frame_id = ~0ull;      // frame_id of the frame sky_out was resolved from (a slot position is reused: an older frame's image is stale)
    uint32_t* disp_out = nullptr;       // RGBA8 sRGB image of the display pass (allocated on first use)
    uint64_t disp_frame_id = ~0ull;     // frame_id of the frame disp_out was resolved from (the sky image's rule)
    uint64_t frame_id = 0;              // frame_counter value of the frame held here
    int row_variant = -1;               // which ordering of the level rows this frame classifies in (Level::d_rows_near), -1: ascending
};

// One batch in flight: a HIP stream, the frames of the batch (frames_per_batch of them) and the argument block of its
// launches.  dev_render stages a frame (host work only); the launches of the whole batch are enqueued when the batch is
// full or flushed, each launch covering all staged frames.
struct Slot {
    hipStream_t stream = nullptr;
    bool owns_stream = true;            // false: the stream belongs to an earlier slot (more slots than hardware queues)
    hipEvent_t done = nullptr;          // recorded after the slot's last launch
    hipEvent_t uploaded = nullptr;      // recorded after the argument block of the slot's batch has been copied to the device
    bool used = false;                  // `uploaded` has been recorded at least once
    std::vector<FrameRes> fr;
    uint32_t pending = 0;               // frames staged and not launched yet
    int method = 0; int models = 0;        // kernel variant of the staged frames (a batch is homogeneous); models: 0 none, 1 in flat space only, 2 lensed (launch_trace)
    uint32_t* d_qctl = nullptr;         // [frames_per_batch][BHRAY_QCTL_WORDS]
    uint32_t launched_frames = 0;       // frames of the batch launched last from this slot (their work counters are valid once it has completed)
    Counters64* d_counters = nullptr;   // [frames_per_batch][BHRAY_MAX_LEVELS]
    uint8_t* h_args = nullptr;          // pinned staging of the argument block: FrameParams[B], then FrameLaunch[B] per launch
    uint8_t* d_args = nullptr;
    size_t args_cap = 0;
    uint64_t batch_id = 0;              // batch_counter value of the batch this slot holds
    uint2* post_scratch = nullptr;      // display pass: bloom levels + tone-mapped image (allocated on first use; the frames of a slot run in stream order)
    // trace grids by queue length (launch_batch): [frames_per_batch][BHRAY_LEVEL_GRID_LAUNCHES] words in pinned memory, written by the trace launches (FrameLaunch::qlen):
    // the rays the queue of that slot position and ladder launch held the last time it ran; QLEN_NONE: nothing reported
    uint32_t* h_qlen = nullptr;
    int qlen_method = -1, qlen_models = -1;             // the kernel variant the words were reported by (another variant: they are reset)
    bhray_level_grid_info grids{};                      // the batch launched last from this slot (dev_get_level_grids; the totals are the ctx's)
};
constexpr uint32_t QLEN_NONE = 0xFFFFFFFFu;

struct ModelStore {
    float pos[3] = {0, 0, 0};
    int visible = 0;
    float4* points = nullptr; float4* normals = nullptr; int32_t* triangles = nullptr;
    float4* nodes = nullptr; int32_t* lookup = nullptr; float4* leaf = nullptr;
    int point_count = 0, normal_count = 0, triangle_count = 0, node_count = 0;
    int root_cull = 0; float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};   // union of the root's child boxes (ModelDev)
    bool loaded = false;
    // a slot built on the device (dev_upload_model_build): the builder's scratch, kept for dev_update_model_vertices; nodes has room for 2 T - 1
    BvhBuild* build = nullptr;
    BvhResult* d_result = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};     // before the copies, between copies and build, behind the build
    bhray_model_build_info info{};
    // the affine pose of DESIGN.md §14: the rest arrays (allocated by the slot's first dev_set_model_pose) and the pose in force; points / normals are then
    // what launch_bvh_pose makes of them
    float4* rest_points = nullptr; float4* rest_normals = nullptr;
    bool posed = false; float pose[12] = {0};
};

}  // namespace

struct bhray_dev {
    bhray_config cfg{};
    int device = 0;
    std::vector<Level> levels;
    std::vector<Slot> slots;               // batches in flight
    uint32_t batch = 1;                    // frames per batch
    int last_slot = 0, last_sub = 0;       // slot / position in its batch of the most recently rendered frame
    uint64_t batch_counter = 0;            // batches launched so far; the staging slot is batch_counter % slots
    uint64_t retired = 0;                  // batches known to have completed (polled oldest-first at every launch): batch_counter - retired are in flight
    int dynamic_dense = -1;                // BHRAY_DYNAMIC_DENSE=n overrides the policy below (0: by the slot count; n > 0: by the batches in flight now, threshold n)
    bhray::DevOptions opt;
    float4* bound_out = nullptr;           // dev_bind_output: destination of the next frame (one-shot)
    std::vector<hipEvent_t> waits;         // dev_wait_event: pending dependencies of the next render (events owned by the caller)
    int launched_slot = -1;                // dev_take_launched
    uint32_t launched_frames = 0;
    size_t out_bytes = 0;
    size_t out_alloc = 0;                  // bytes of every frame's own output buffer (>= out_bytes)
    size_t spec_alloc = 0, pred_alloc = 0, super_alloc = 0;   // entries of the merged queues (speculative / temporal / superset modes)
    std::vector<uint32_t> local_rows;      // frame rows of this partition, increasing
    size_t row_work_off[BHRAY_MAX_LEVELS + 1] = {0};   // BHRAY_F_COUNTERS: offset of every level's rows in FrameRes::d_row_work; [levels] = total
    // scene
    uint8_t* tex[3] = {nullptr, nullptr, nullptr};
    int tex_w[3] = {0, 0, 0}, tex_h[3] = {0, 0, 0};
    int sky_filter = 0;                    // dev_set_sky_filter: 1 = dev_resolve_sky runs the footprint filter
    uint2* pyr_buf = nullptr;              // ... and the sky texture's pyramid, levels 1 .. top: held only while the mode is on
    bhray::SkyPyr pyr{};
    float4* star_buf = nullptr;            // dev_set_stars: the catalogue sorted by cell, two float4 per star; held only while a catalogue is set
    uint32_t* star_prefix = nullptr;       // ... and its cells' prefix array
    bhray::StarSet stars{};                // what star_kernel reads; stars.stars == nullptr: no catalogue, dev_resolve_sky launches nothing more
    uint32_t star_count = 0;
    ModelStore models[BHRAY_MAX_MODELS];
    bhray_camera_uniform cam{};
    bhray_black_hole_uniform bh{};
    bhray_details det{};
    bool have_uniforms = false;
    bool mesh_lensing = false;             // dev_set_mesh_lensing: models are tested on every step inside the relativity sphere too (from the next dev_render)
    bool lens_rays = false;                // ... its BHRAY_LENS_RAYS bit: and in ray batches, ray records and what bhray_accum_* traces (from the next batch enqueued)
    std::vector<hipEvent_t> events;        // ring: [BHRAY_TIMING_RING][events_per_batch(levels)], indexed by ev_* (batch_events)
    uint64_t frame_counter = 0, timing_begin = 0;   // timing_begin: first batch not yet reported by dev_get_timing
    uint8_t sky_recorded[BHRAY_TIMING_RING] = {0};
    uint8_t ring_frames[BHRAY_TIMING_RING] = {0};   // frames of the batch held by each timing-ring entry
    uint8_t ring_own_trace[BHRAY_TIMING_RING] = {0};   // ... and its levels that had a trace launch of their own (bit l; BatchPlan::own_trace)
    // execution spans of the trace launches of timed batches (FrameLaunch::span): [BHRAY_TIMING_RING][SPAN_MAX][2] device words
    unsigned long long* d_span = nullptr;
    uint8_t ring_spans[BHRAY_TIMING_RING] = {0};    // trace launches of each timing-ring entry
    double wall_clock_khz = 100000.0;               // hipDeviceAttributeWallClockRate (s_memrealtime: 100 MHz on gfx950)
    int* d_err = nullptr;
    int num_cus = 256;
    // BHRAY_F_TEMPORAL: what is predicted beyond the pixels the previous frame traced (measured at 1080p on a camera orbiting at 0.002
    // and 0.02 rad per frame, profiles/r02_experiments.json "temporal_prediction"): interpolated pixels whose widest neighbour angle
    // exceeded 0.8 x the threshold, pixels within 4 (levels below the last) / 1 (last level) pixels of a predicted one, and the clamped
    // border pixels (predict_kernel).  +8 % rays; the levels below the last then miss nothing, the last level a few hundred aliased
    // pixels: ONE fix-up launch instead of three.  BHRAY_TEMPORAL_MARGIN / BHRAY_TEMPORAL_RADIUS="last[,below]" override (tuning).
    float temporal_margin = 0.8f;
    uint32_t temporal_radius_coarse = 4;
    uint32_t temporal_radius = 1;
                                           // radius of 1-2 adds 2-4 % rays and does not shorten a moving camera's frames - the misses are scattered interpolate/trace flips)
    int bpc_override = 0;                  // BHRAY_TRACE_BLOCKS_PER_CU (tuning experiments only)
    int grid_override = 0;                 // BHRAY_TRACE_GRID: absolute number of persistent trace blocks (tuning experiments only)
    int wave_prio = -1;                    // BHRAY_PRIO=0/1 forces wave priority off / on for every latency-build launch; -1 = one frame per launch and ONE frame slot
    int quad_wps = -1;                     // BHRAY_QUAD: waves per SIMD the quad march may use for a short queue (bhray_quad.inc); 0 = the scalar thin shares only; -1 = the measured default (RK 2, Euler 1)
    int dense_override = -1;               // BHRAY_TRACE_DENSE=0/1 (tuning experiments only)
    int coarse_build = -1;                 // BHRAY_COARSE_BUILD=0/1 (experiment): the build of the trace launches below the ladder's last level (-1: the batch's build)
    int origin_kernel = 1;                 // BHRAY_ORIGIN_KERNEL=0: never the ORIGIN builds of the trace kernels (the A/B of EXPERIMENTS R10.1; the same pixels)
    // BHRAY_LEVEL_GRID / _GEN / _MARGIN / _FLOOR: dense ladder trace launches get a grid sized by the rays their queues held last time (bhray_trace_grid_for)
    int level_grid = 1; uint32_t level_grid_gen = 256, level_grid_margin = 25, level_grid_floor = 64;
    uint64_t grid_launches = 0, grid_blocks = 0, grid_ceiling_launches = 0;   // ladder trace launches enqueued, their blocks, those with the ctx's grid (dev_get_level_grids)
    uint64_t origin_launches = 0, general_launches = 0;      // trace launches enqueued with an ORIGIN build / with any other (dev_get_trace_builds)
    bool rendered = false;
    // ray batches (dev_trace_rays / dev_trace_rays_device): a stream of their own, created by the first batch - a ctx that only renders frames keeps the
    // streams it had -, the events that order a batch against the caller's stream, the argument block of one launch (FrameParams, FrameLaunch and the two queue control
    // words: pinned, and its device copy) and the host variant's grow-only staging (pinned in / out, device in / out)
    hipStream_t q_stream = nullptr;
    hipEvent_t q_begin = nullptr, q_done = nullptr, q_uploaded = nullptr;
    uint8_t* q_hargs = nullptr; uint8_t* q_dargs = nullptr;
    bool q_used = false;                   // a batch has been enqueued (q_uploaded has been recorded; the engine's error word may be a batch's)
    float4* q_hin = nullptr; float4* q_hout = nullptr; float4* q_din = nullptr; float4* q_dout = nullptr;
    size_t q_cap = 0;                      // rays the staging holds
    bhray_ray_record* q_hrec = nullptr; bhray_ray_record* q_drec = nullptr;      // the records' staging (bhray_trace_rays_records): grow-only, allocated by the first records batch
    size_t q_rec_cap = 0;
    bhray_path_point* q_hpts = nullptr; bhray_path_point* q_dpts = nullptr;      // the paths' staging (bhray_trace_rays_paths): grow-only, allocated by the first paths batch
    uint32_t* q_hcnt = nullptr; uint32_t* q_dcnt = nullptr;
    size_t q_pts_cap = 0, q_cnt_cap = 0;   // points / rays the staging holds
    // the accumulation image (dev_accum_*): allocated by the first dev_accum_begin; everything runs on q_stream
    float4* a_sum = nullptr; float4* a_mean = nullptr;       // frame_w * frame_h each: (sum of colours, samples taken), and the mean of the last read
    uint2* a_mean16 = nullptr; uint2* a_scratch = nullptr; uint32_t* a_disp = nullptr;   // the display read: the mean as RGBA16F, the display pass's scratch, its RGBA8 image (first dev_accum_read_display)
    float4* a_rays = nullptr; float4* a_res = nullptr;       // one launch's generated records (2 float4 each) and results: grow-only (the stream is idle when they grow)
    size_t a_cap = 0;                      // rays that staging holds
    uint32_t a_samples = 0;                // sample indices enqueued since the last begin: the next add starts there
    // still passes (dev_accum_set_passes): nothing below is allocated while every accumulation's set is 0
    uint32_t a_passes_next = 0;            // the stored set: dev_accum_begin copies it
    uint32_t a_passes = 0;                 // the set of the current accumulation (0 before the first begin)
    float4* a_pass[ACCUM_PASS_COUNT] = {}; // one sum plane per pass, frame_w * frame_h: allocated by the first begin that carries the pass
    float4* a_rec = nullptr; size_t a_rec_cap = 0;           // one launch's ray records (2 float4 each), beside a_rays / a_res: grow-only
    float4* a_pimg = nullptr; size_t a_pimg_cap = 0;         // one pass's sample images of a launch under a tent or a cubic: grow-only
    // denoised stills (dev_accum_read_denoised): the filter's working images, frame_w * frame_h texels each, allocated by the first read that needs them
    float4* a_dn[2] = {};                  // the two ping-pong images (r, g, b, t)
    float4* a_dng[3] = {};                 // the packed guide means: (coverage xyz, closest), position xyz, escape xyz
    uint32_t a_launch_rays = 0;            // dev_accum_set_launch_rays: rays per trace launch (0: BHRAY_ACCUM_LAUNCH_RAYS)
    bool a_begun = false;
    // adaptive stills (dev_accum_add_adaptive): allocated by the first adaptive call or selection; everything runs on q_stream
    uint4* a_state = nullptr;              // frame_w * frame_h records (S1, S2, issued, 0) beside a_sum
    uint32_t* a_list = nullptr;            // the selection's compacted pixel indices, frame_w * frame_h words; the counts read's staging too
    uint32_t* a_ctl = nullptr; uint32_t* a_hctl = nullptr;   // the selection's control block ([0] count, [1] largest issued): device, and the pinned word it is copied to
    int a_mode = 0;                        // since the last begin: 0 no sample yet, 1 dev_accum_add's, 2 adaptive (a_samples is then `reach`)
    uint32_t a_min = 0, a_round = 0;       // the first adaptive call's min_samples / round_samples since begin: what later calls must repeat
    // still cameras (dev_accum_set_camera): read by every dev_accum_add / dev_accum_add_adaptive / dev_accum_sample_rays at the time of the call
    bhray_still_camera a_cam{(uint32_t)sizeof(bhray_still_camera), BHRAY_STILL_PINHOLE, 3.14159274f, 0.0f, 1.0f};
    // still pixel filters (dev_accum_set_filter): read by every dev_accum_add at the time of the call; the box runs accum_add_kernel
    bhray_still_filter a_filter{(uint32_t)sizeof(bhray_still_filter), BHRAY_FILTER_BOX, 2.0f, 1.0f / 3.0f, 1.0f / 3.0f};
    // point stars in stills (dev_accum_set_stars): read by every dev_accum_add at the time of the call; acts only while a catalogue is in force (stars)
    bool a_stars = false;
    // the moving observer (dev_accum_set_observer): read like a_cam; an all-zero velocity is "no observer"
    bhray_observer a_obs{(uint32_t)sizeof(bhray_observer), {0.0f, 0.0f, 0.0f}, 1u};
    bhray::ReadRing reads;                 // tickets of the asynchronous hand-off (dev_read_async)
    std::string err;
};

namespace {

hipEvent_t* batch_events(bhray_dev* c, size_t ring) { return &c->events[ring * events_per_batch(c->cfg.levels)]; }

int fail(bhray_dev* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail(ctx, BHRAY_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

}  // namespace
// rows of level k-1 that the rows `fine` of level k read (ray.wgsl:185-201), same binary32 math
std::vector<int32_t> bhray::coarse_rows_needed(const std::vector<int32_t>& fine, int h, int ph) {
    std::vector<uint8_t> need((size_t)ph, 0);
    if (ph == 1) return {};
    const int sf = (h - 1) / (ph - 1);
    const float ry = (float)ph / (float)(h + (sf - 1));
    for (int32_t y : fine) {
        const float ppy = (float)y * ry;
        int tl = (int)floorf(ppy);
        int a = tl < 0 ? 0 : (tl > ph - 1 ? ph - 1 : tl);
        int b = tl + 1; b = b < 0 ? 0 : (b > ph - 1 ? ph - 1 : b);
        need[(size_t)a] = 1; need[(size_t)b] = 1;
    }
    std::vector<int32_t> out;
    for (int y = 0; y < ph; y++) if (need[(size_t)y]) out.push_back(y);
    return out;
}
namespace {

// bh_acos(c) < thr  <=>  c > acos_threshold(thr)  for c in [-1, 1]: bh_acos is monotone non-increasing over all binary32 values
// of the interval (exhaustive check: dev_selftest), so the set where the predicate holds is an upper interval; its lower end is
// found by bisection over the ordered bit patterns with the same bh_acos the kernels use.
float acos_threshold(float thr) {
    if (!(thr == thr)) return INFINITY;                              // NaN threshold: never smaller
    if (!(bh_acos(1.0f) < thr)) return INFINITY;                     // not even angle 0 is below the threshold
    if (bh_acos(-1.0f) < thr) return u2f(0xbf800001u);               // every c of [-1, 1] is: c > (largest float below -1)
    // ordered keys: k < 0 <-> x = -|bits|, k >= 0 <-> x = +bits; x(k) increasing in k
    auto xk = [](int64_t k) { return k >= 0 ? u2f((uint32_t)k) : u2f(0x80000000u | (uint32_t)(-k)); };
    int64_t lo = -(int64_t)0x3f800000, hi = (int64_t)0x3f800000;     // predicate false at lo (x = -1), true at hi (x = 1)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (bh_acos(xk(mid)) < thr) hi = mid; else lo = mid;
    }
    return xk(lo);                                                   // the largest c whose angle is not below the threshold
}

void derive_frame(const bhray_dev* c, FrameParams& P) {
    memset(&P, 0, sizeof P);
    const bhray_camera_uniform& cam = c->cam;
    const bhray_black_hole_uniform& bh = c->bh;
    const bhray_details& d = c->det;
    const F3 fwd = ld3(cam.forward);
    const F3 plane_up = f3(0.0f, -1.0f, 0.0f);
    const F3 right = normalize(cross(fwd, plane_up));               // ray.wgsl:276
    const F3 up = normalize(cross(fwd, right));                     // ray.wgsl:277
    const float fov_factor = 1.0f / bh_tan(cam.fov / 2.0f);         // ray.wgsl:279
    const F3 fwd_ff = fwd * fov_factor;
    const F3 cpos = ld3(cam.position), bpos = ld3(bh.position);
    P.cam[0] = cpos.x; P.cam[1] = cpos.y; P.cam[2] = cpos.z;
    P.right[0] = right.x; P.right[1] = right.y; P.right[2] = right.z;
    P.up[0] = up.x; P.up[1] = up.y; P.up[2] = up.z;
    P.fwd_ff[0] = fwd_ff.x; P.fwd_ff[1] = fwd_ff.y; P.fwd_ff[2] = fwd_ff.z;
    P.ray_distance = distance(cpos, bpos);
    P.ray_distance_f = fdistance(cpos, bpos);
    P.relativity0 = P.ray_distance < bh.relativity_sphere_radius ? 1 : 0;
    P.bh[0] = bpos.x; P.bh[1] = bpos.y; P.bh[2] = bpos.z;
    memcpy(P.bn, bh.normal, 12);
    P.bn_len = length(ld3(bh.normal));
    P.cull_outer_pad = bh.accretion_disk_outer + 0.0501f; P.cull_plane_c1 = 1.0101f * P.bn_len; P.cull_plane_c2 = 1.01e-4f * P.bn_len;
    P.inner = bh.accretion_disk_inner; P.outer = bh.accretion_disk_outer;
    P.rot_speed = bh.rotation_speed; P.R = bh.relativity_sphere_radius;
    P.show_tex = bh.show_disk_texture; P.show_shift = bh.show_red_shift;
    for (int col = 0; col < 3; col++) for (int r = 0; r < 3; r++) P.M[3 * col + r] = bh.rotation_matrix[4 * col + r];
    P.feather = bh.feather_amount;
    P.time = d.time; P.time_rot = d.time * bh.rotation_speed; P.method = d.integration_method != 0 ? 1 : 0; P.step_size = d.step_size;
    P.max_iter = d.max_iterations; P.thr = d.angle_division_threshold;
    P.acos_cstar = acos_threshold(P.thr);
    P.acos_cstar_near = c->temporal_margin < 1.0f ? acos_threshold(P.thr * c->temporal_margin) : P.acos_cstar;
    int mc = d.model_count; if (mc < 0) mc = 0; if (mc > BHRAY_MAX_MODELS) mc = BHRAY_MAX_MODELS;
    // Every slot below model_count is built; one never uploaded, one with 0 triangles and an invisible one get visible = 0 (the kernels
    // skip it, as ray.wgsl:378 skips a default ModelUniform).  The kernels loop to the highest such slot that is visible, + 1.
    int usable = 0;
    for (int i = 0; i < mc; i++) {
        const ModelStore& m = c->models[i];
        ModelDev& md = P.models[i];
        memcpy(md.pos, m.pos, 12);
        md.visible = (m.loaded && m.triangle_count > 0) ? m.visible : 0;
        md.points = m.points; md.normals = m.normals; md.triangles = m.triangles; md.nodes = m.nodes; md.lookup = m.lookup; md.leaf = m.leaf;
        md.node_count = m.node_count;
        md.root_cull = m.root_cull; memcpy(md.root_lo, m.root_lo, 12); memcpy(md.root_hi, m.root_hi, 12);
        if (md.visible != 0) usable = i + 1;
    }
    P.model_count = usable;                  // 0 when no slot is visible: nothing to traverse, the no-mesh kernel variant is exact
    TexDev* t[3] = {&P.temp, &P.disk, &P.sky};
    for (int i = 0; i < 3; i++) { t[i]->rgba = c->tex[i]; t[i]->w = c->tex_w[i]; t[i]->h = c->tex_h[i]; }
}

int launch_batch(bhray_dev* c);

// everything the engine has enqueued: the frames in flight and the outstanding ray batches (both read the scene memory the callers of this rewrite)
hipError_t sync_all(bhray_dev* c) {
    for (Slot& S : c->slots) {
        hipError_t e = hipStreamSynchronize(S.stream);
        if (e != hipSuccess) return e;
    }
    if (c->q_stream) return hipStreamSynchronize(c->q_stream);
    return hipSuccess;
}

void free_model(ModelStore& m) {
    if (m.points) (void)hipFree(m.points);
    if (m.normals) (void)hipFree(m.normals);
    if (m.triangles) (void)hipFree(m.triangles);
    if (m.nodes) (void)hipFree(m.nodes);
    if (m.lookup) (void)hipFree(m.lookup);
    if (m.leaf) (void)hipFree(m.leaf);
    if (m.d_result) (void)hipFree(m.d_result);
    if (m.rest_points) (void)hipFree(m.rest_points);
    if (m.rest_normals) (void)hipFree(m.rest_normals);
    bvh_build_destroy(m.build);
    for (hipEvent_t e : m.ev) if (e) (void)hipEventDestroy(e);
    m = ModelStore();
}

}  // namespace

extern "C" {

const char* bhray_strerror(int code) {
    switch (code) {
        case BHRAY_OK: return "ok";
        case BHRAY_E_INVALID: return "invalid argument";
        case BHRAY_E_NO_DEVICE: return "no usable HIP device";
        case BHRAY_E_HIP: return "HIP runtime error";
        case BHRAY_E_NOMEM: return "out of memory";
        case BHRAY_E_STATE: return "call order violated";
        case BHRAY_E_BVH_DEPTH: return "BVH deeper than the traversal stack";
        case BHRAY_E_IO: return "I/O or parse error";
        case BHRAY_E_CAPACITY: return "model exceeds reference capacity";
        case BHRAY_E_COMM: return "RCCL unavailable or collective failed";
        default: return "unknown error";
    }
}

uint32_t bhray_version(void) { return (BHRAY_VERSION_MAJOR << 16) | BHRAY_VERSION_MINOR; }


int bhray_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// bhray_diag.h: the display pass over a caller's image - no ctx.  Allocate, copy in, the product's launch_display (or launch_fxaa), wait, copy out, free.
int bhray_diag_display_image(int device, const uint16_t* rgba16f, uint32_t w, uint32_t h, const void* fxaa16, const void* mix4, uint32_t flags,
                             uint8_t* dst_rgba8, uint16_t* stages_rgba16f, size_t stage_texels) {
    if (!rgba16f || !dst_rgba8) return fail(nullptr, BHRAY_E_INVALID, "bhray_diag_display_image: NULL image or destination");
    if (flags & ~(uint32_t)BHRAY_DIAG_DISPLAY_FXAA_ONLY) return fail(nullptr, BHRAY_E_INVALID, "bhray_diag_display_image: unknown flag bits 0x%x", flags);
    const bool fxaa_only = (flags & BHRAY_DIAG_DISPLAY_FXAA_ONLY) != 0;
    const size_t scratch_bytes = display_scratch_bytes(w, h);
    if (scratch_bytes == 0 || w > 32767 || h > 32767)               // the ladder's largest frame: the kernels index pixels with an int
        return fail(nullptr, BHRAY_E_INVALID, "bhray_diag_display_image: the display pass takes frames from 32 x 32 to 32767 x 32767 pixels (got %u x %u)", w, h);
    bhray_fxaa_details fx; bhray_mix_details mx;
    (void)bhray_post_defaults(&fx, &mx);
    if (fxaa16) memcpy(&fx, fxaa16, sizeof fx);
    if (mix4) memcpy(&mx, mix4, sizeof mx);
    if (fx.iterations > BHRAY_FXAA_MAX_ITERATIONS)
        return fail(nullptr, BHRAY_E_INVALID, "fxaa iterations %d > BHRAY_FXAA_MAX_ITERATIONS (%d)", fx.iterations, BHRAY_FXAA_MAX_ITERATIONS);
    if (stages_rgba16f && fxaa_only) return fail(nullptr, BHRAY_E_INVALID, "bhray_diag_display_image: BHRAY_DIAG_DISPLAY_FXAA_ONLY has no stage output");
    if (stages_rgba16f && stage_texels != scratch_bytes / sizeof(uint2))
        return fail(nullptr, BHRAY_E_INVALID, "bhray_diag_display_image: the stage output of a %u x %u frame is %zu texels, not %zu", w, h, scratch_bytes / sizeof(uint2), stage_texels);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, BHRAY_E_NO_DEVICE, "no HIP device visible (libbhray has no CPU path)");
    if (device < 0 || device >= ndev) return fail(nullptr, BHRAY_E_NO_DEVICE, "device %d not present (%d visible)", device, ndev);
    const size_t npix = (size_t)w * h;
    uint2 *d_in = nullptr, *d_scratch = nullptr;
    uint32_t* d_out = nullptr;
    const char* what = "hipSetDevice";
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) { what = "hipMalloc"; e = hipMalloc(&d_in, npix * sizeof(uint2)); }
    if (e == hipSuccess) e = hipMalloc(&d_out, npix * sizeof(uint32_t));
    if (e == hipSuccess && !fxaa_only) e = hipMalloc(&d_scratch, scratch_bytes);
    if (e == hipSuccess) { what = "hipMemcpy"; e = hipMemcpy(d_in, rgba16f, npix * sizeof(uint2), hipMemcpyHostToDevice); }
    if (e == hipSuccess) {
        what = fxaa_only ? "launch_fxaa" : "launch_display";
        e = fxaa_only ? launch_fxaa(d_in, d_out, w, h, fx, nullptr) : launch_display(d_in, d_scratch, d_out, w, h, fx, mx, nullptr);
    }
    if (e == hipSuccess) { what = "hipStreamSynchronize"; e = hipStreamSynchronize(nullptr); }
    if (e == hipSuccess) { what = "hipMemcpy"; e = hipMemcpy(dst_rgba8, d_out, npix * sizeof(uint32_t), hipMemcpyDeviceToHost); }
    if (e == hipSuccess && stages_rgba16f) e = hipMemcpy(stages_rgba16f, d_scratch, scratch_bytes, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (d_scratch) (void)hipFree(d_scratch);
    if (e != hipSuccess) return fail(nullptr, e == hipErrorOutOfMemory ? BHRAY_E_NOMEM : BHRAY_E_HIP, "bhray_diag_display_image: %s: %s", what, hipGetErrorString(e));
    return BHRAY_OK;
}

int bhray_ladder_from_base(uint32_t base_w, uint32_t base_h, uint32_t m, uint32_t levels, bhray_config* cfg) {
    if (!cfg || levels < 1 || levels > BHRAY_MAX_LEVELS || base_w < 2 || base_h < 2 || m < 2) return BHRAY_E_INVALID;
    uint64_t w = base_w, h = base_h;
    for (uint32_t i = 0; i < levels; i++) {
        if (w > 32767 || h > 32767) return BHRAY_E_INVALID;          // queue entries pack tag<<30 | y<<15 | x
        cfg->level_w[i] = (uint32_t)w; cfg->level_h[i] = (uint32_t)h;
        w = w * m - (m - 1); h = h * m - (m - 1);                    // mod.rs:203-204
    }
    cfg->levels = levels;
    cfg->crop_x = 0; cfg->crop_y = 0;
    cfg->frame_w = cfg->level_w[levels - 1]; cfg->frame_h = cfg->level_h[levels - 1];
    if (cfg->row_world == 0) { cfg->row_world = 1; cfg->row_rank = 0; }
    if (cfg->stripe_rows == 0) cfg->stripe_rows = 27;
    cfg->struct_size = sizeof(bhray_config);
    return BHRAY_OK;
}

int bhray_ladder_for_frame(uint32_t frame_w, uint32_t frame_h, uint32_t m, uint32_t levels, bhray_config* cfg) {
    if (!cfg || levels < 1 || levels > BHRAY_MAX_LEVELS || frame_w < 2 || frame_h < 2 || m < 2) return BHRAY_E_INVALID;
    uint64_t s = 1;
    for (uint32_t i = 1; i < levels; i++) s *= m;                    // last = (base-1)*m^(levels-1) + 1
    const uint64_t bw = (frame_w - 1 + s - 1) / s + 1, bh_ = (frame_h - 1 + s - 1) / s + 1;
    int rc = bhray_ladder_from_base((uint32_t)(bw < 2 ? 2 : bw), (uint32_t)(bh_ < 2 ? 2 : bh_), m, levels, cfg);
    if (rc) return rc;
    const uint32_t lw = cfg->level_w[levels - 1], lh = cfg->level_h[levels - 1];
    cfg->crop_x = (lw - frame_w) / 2; cfg->crop_y = (lh - frame_h) / 2;
    cfg->frame_w = frame_w; cfg->frame_h = frame_h;
    return BHRAY_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// per-device engine (bhray_dev.h): one partition of the frame on one GPU.  The public bhray_ctx (bhray_group.hip) owns one
// of these per local partition.
// ------------------------------------------------------------------------------------------
const char* dev_last_error(const bhray_dev* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
void dev_set_create_error(const char* msg) { g_create_error = msg ? msg : ""; }

void dev_destroy(bhray_dev* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (Slot& S : c->slots) if (S.stream) (void)hipStreamSynchronize(S.stream);
    if (c->q_stream) (void)hipStreamSynchronize(c->q_stream);
    if (c->q_hargs) (void)hipHostFree(c->q_hargs);
    if (c->q_dargs) (void)hipFree(c->q_dargs);
    if (c->q_hin) (void)hipHostFree(c->q_hin);
    if (c->q_hout) (void)hipHostFree(c->q_hout);
    if (c->q_din) (void)hipFree(c->q_din);
    if (c->q_dout) (void)hipFree(c->q_dout);
    if (c->q_hrec) (void)hipHostFree(c->q_hrec);
    if (c->q_drec) (void)hipFree(c->q_drec);
    if (c->q_hpts) (void)hipHostFree(c->q_hpts);
    if (c->q_dpts) (void)hipFree(c->q_dpts);
    if (c->q_hcnt) (void)hipHostFree(c->q_hcnt);
    if (c->q_dcnt) (void)hipFree(c->q_dcnt);
    for (void* p : {(void*)c->a_sum, (void*)c->a_mean, (void*)c->a_mean16, (void*)c->a_scratch, (void*)c->a_disp, (void*)c->a_rays, (void*)c->a_res, (void*)c->a_state, (void*)c->a_list, (void*)c->a_ctl, (void*)c->a_rec, (void*)c->a_pimg,
                    (void*)c->a_pass[0], (void*)c->a_pass[1], (void*)c->a_pass[2], (void*)c->a_pass[3],
                    (void*)c->a_dn[0], (void*)c->a_dn[1], (void*)c->a_dng[0], (void*)c->a_dng[1], (void*)c->a_dng[2]}) if (p) (void)hipFree(p);
    if (c->a_hctl) (void)hipHostFree(c->a_hctl);
    for (hipEvent_t e : {c->q_begin, c->q_done, c->q_uploaded}) if (e) (void)hipEventDestroy(e);
    if (c->q_stream) (void)hipStreamDestroy(c->q_stream);
    for (Slot& S : c->slots) {
        for (FrameRes& R : S.fr) {
            for (auto p : R.level_out) if (p) (void)hipFree(p);
            for (auto p : R.queue) if (p) (void)hipFree(p);
            for (auto p : R.spec_out) if (p) (void)hipFree(p);
            if (R.spec_queue) (void)hipFree(R.spec_queue);
            if (R.super_queue) (void)hipFree(R.super_queue);
            if (R.pred_queue) (void)hipFree(R.pred_queue);
            for (auto p : R.need) if (p) (void)hipFree(p);
            for (auto p : R.stamp) if (p) (void)hipFree(p);
            if (R.own_out) (void)hipFree(R.own_out);
            if (R.d_row_work) (void)hipFree(R.d_row_work);
            if (R.sky_out) (void)hipFree(R.sky_out);
            if (R.disp_out) (void)hipFree(R.disp_out);
        }
        if (S.post_scratch) (void)hipFree(S.post_scratch);
        if (S.d_qctl) (void)hipFree(S.d_qctl);
        if (S.d_counters) (void)hipFree(S.d_counters);
        if (S.h_args) (void)hipHostFree(S.h_args);
        if (S.h_qlen) (void)hipHostFree(S.h_qlen);
        if (S.d_args) (void)hipFree(S.d_args);
        if (S.done) (void)hipEventDestroy(S.done);
        if (S.uploaded) (void)hipEventDestroy(S.uploaded);
        if (S.stream && S.owns_stream) (void)hipStreamDestroy(S.stream);
    }
    for (Level& L : c->levels) {
        if (L.d_rows) (void)hipFree(L.d_rows);
        if (L.d_rows_near) (void)hipFree(L.d_rows_near);
        if (L.d_rowmap) (void)hipFree(L.d_rowmap);
    }
    for (auto& t : c->tex) if (t) (void)hipFree(t);
    if (c->pyr_buf) (void)hipFree(c->pyr_buf);
    if (c->star_buf) (void)hipFree(c->star_buf);
    if (c->star_prefix) (void)hipFree(c->star_prefix);
    for (auto& m : c->models) free_model(m);
    for (auto& e : c->events) if (e) (void)hipEventDestroy(e);
    if (c->d_err) (void)hipFree(c->d_err);
    if (c->d_span) (void)hipFree(c->d_span);
    c->reads.destroy();
    delete c;
}

namespace {
// The partition's rows (bhray_config.partition of c->cfg), the level rows they depend on (top-down, ray.wgsl:185-201), and their
// device tables.  The tables are allocated for a whole level, so a partition set later (dev_set_partition) rewrites them in place.
int build_row_tables(bhray_dev* c) {
    const bhray_config* cfg = &c->cfg;
    const uint32_t nl = cfg->levels;
    c->local_rows = partition_row_list(*cfg, cfg->row_world, cfg->row_rank);
    for (uint32_t l = 0; l < nl; l++) c->levels[l].rows.clear();
    {
        Level& F = c->levels[nl - 1];
        for (uint32_t r : c->local_rows) F.rows.push_back((int32_t)(cfg->crop_y + r));
        for (int l = (int)nl - 1; l > 0; l--)
            c->levels[l - 1].rows = coarse_rows_needed(c->levels[l].rows, c->levels[l].h, c->levels[l - 1].h);
    }
    for (uint32_t l = 0; l < nl; l++) {
        Level& L = c->levels[l];
        const bool last = (l == nl - 1);
        const size_t nrows = L.rows.size();
        if (!L.d_rows) HIPCHK(c, hipMalloc(&L.d_rows, (size_t)L.h * sizeof(int32_t)));
        if (nrows) {
            HIPCHK(c, hipMemcpy(L.d_rows, L.rows.data(), nrows * sizeof(int32_t), hipMemcpyHostToDevice));
            if (BHRAY_ROW_VARIANTS >= 2) {
                // The same rows with the tile rows (8 list entries) nearest a centre row first: the rays that pass closest to the hole are the
                // longest, and a launch lasts as long as its last rays - classified first they enter the queue first and are traced first
                // (every pixel is classified independently of the others: the order changes nothing else).  One ordering per centre row;
                // a frame picks the one nearest the row the hole projects to (dev_render).
                const size_t nch = nrows / 8;                         // whole tile rows; a short last one stays last
                std::vector<int32_t> all((size_t)BHRAY_ROW_VARIANTS * nrows);
                for (int v = 0; v < BHRAY_ROW_VARIANTS; v++) {
                    const double centre = (double)v / (double)(BHRAY_ROW_VARIANTS - 1) * (double)(L.h - 1);
                    std::vector<size_t> ch(nch);
                    for (size_t k = 0; k < nch; k++) ch[k] = k;
                    std::stable_sort(ch.begin(), ch.end(), [&](size_t a, size_t b) {
                        return fabs((double)L.rows[a * 8 + 4] - centre) < fabs((double)L.rows[b * 8 + 4] - centre);
                    });
                    int32_t* o = all.data() + (size_t)v * nrows;
                    size_t n = 0;
                    for (size_t k : ch) for (size_t j = k * 8; j < k * 8 + 8; j++) o[n++] = L.rows[j];
                    for (size_t j = nch * 8; j < nrows; j++) o[n++] = L.rows[j];
                }
                if (!L.d_rows_near) HIPCHK(c, hipMalloc(&L.d_rows_near, (size_t)BHRAY_ROW_VARIANTS * (size_t)L.h * sizeof(int32_t)));
                HIPCHK(c, hipMemcpy(L.d_rows_near, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            }
        }
        const size_t span = last ? cfg->frame_w : (size_t)L.w;
        L.queue_cap = nrows * span;
        if (last) {
            std::vector<int32_t> map((size_t)L.h, -1);
            for (size_t i = 0; i < c->local_rows.size(); i++) map[(size_t)(cfg->crop_y + c->local_rows[i])] = c->opt.frame_rowmap ? (int32_t)c->local_rows[i] : (int32_t)i;
            if (!L.d_rowmap) HIPCHK(c, hipMalloc(&L.d_rowmap, (size_t)L.h * sizeof(int32_t)));
            HIPCHK(c, hipMemcpy(L.d_rowmap, map.data(), (size_t)L.h * sizeof(int32_t), hipMemcpyHostToDevice));
        }
    }
    c->out_bytes = (c->opt.frame_rowmap ? (size_t)cfg->frame_h : c->local_rows.size()) * (size_t)cfg->frame_w * sizeof(float4);
    return BHRAY_OK;
}

// Every frame's ray queues and own output buffer, sized for the current partition.  `headroom` (a partition set at run time): a buffer
// that has to grow grows by a quarter more than needed, so that bounds that keep moving a few rows do not reallocate every time.
int ensure_frame_buffers(bhray_dev* c, bool headroom) {
    const bhray_config* cfg = &c->cfg;
    const uint32_t nl = cfg->levels;
    auto want = [&](size_t need, size_t full) { size_t w = headroom ? need + need / 4 + 64 : need; return w > full ? std::max(full, need) : w; };
    for (uint32_t l = 0; l < nl; l++) {
        Level& L = c->levels[l];
        if (L.queue_cap <= L.queue_alloc) continue;
        const size_t full = (size_t)L.h * (size_t)(l == nl - 1 ? cfg->frame_w : (uint32_t)L.w);
        const size_t n = want(L.queue_cap, full);
        for (Slot& S : c->slots) for (FrameRes& R : S.fr) {
            if (R.queue[l]) { HIPCHK(c, hipFree(R.queue[l])); R.queue[l] = nullptr; }
            HIPCHK(c, hipMalloc(&R.queue[l], n * sizeof(uint32_t)));
        }
        L.queue_alloc = n;
    }
    auto merged = [&](size_t need, size_t& alloc, uint32_t* FrameRes::*member) -> int {
        if (need <= alloc) return BHRAY_OK;
        const size_t n = headroom ? need + need / 4 + 64 : need;
        for (Slot& S : c->slots) for (FrameRes& R : S.fr) {
            if (R.*member) { HIPCHK(c, hipFree(R.*member)); R.*member = nullptr; }
            HIPCHK(c, hipMalloc(&(R.*member), n * sizeof(uint32_t)));
        }
        alloc = n;
        return BHRAY_OK;
    };
    if (cfg->speculative_levels) {
        size_t cap = 0;
        for (uint32_t l = 0; l < cfg->speculative_levels; l++) cap += c->levels[l].queue_cap;
        int rc = merged(cap, c->spec_alloc, &FrameRes::spec_queue); if (rc) return rc;
    }
    if (cfg->flags & BHRAY_F_TEMPORAL) {
        size_t cap = 0;
        for (uint32_t l = 0; l < nl; l++) cap += c->levels[l].queue_cap;
        int rc = merged(cap, c->pred_alloc, &FrameRes::pred_queue); if (rc) return rc;
    }
    if (cfg->superset_levels) {
        size_t cap = 0;
        for (uint32_t l = nl - cfg->superset_levels; l < nl; l++) cap += c->levels[l].queue_cap;
        int rc = merged(cap, c->super_alloc, &FrameRes::super_queue); if (rc) return rc;
    }
    if (!c->opt.external_out && c->out_bytes > c->out_alloc) {
        const size_t full = (size_t)cfg->frame_h * (size_t)cfg->frame_w * sizeof(float4);
        size_t n = headroom ? c->out_bytes + c->out_bytes / 4 : c->out_bytes;
        if (n > full) n = std::max(full, c->out_bytes);
        for (Slot& S : c->slots) for (FrameRes& R : S.fr) {
            if (R.own_out) { HIPCHK(c, hipFree(R.own_out)); R.own_out = nullptr; }
            HIPCHK(c, hipMalloc(&R.own_out, n));
            HIPCHK(c, hipMemset(R.own_out, 0xFF, n));
            R.out = R.own_out;
        }
        c->out_alloc = n;
    }
    return BHRAY_OK;
}
}  // namespace

int dev_create(const bhray_config* cfg, const bhray::DevOptions& opt, bhray_dev** out) {
    if (!cfg || !out) return fail(nullptr, BHRAY_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(bhray_config)) return fail(nullptr, BHRAY_E_INVALID, "bhray_config.struct_size mismatch");
    if (cfg->levels < 1 || cfg->levels > BHRAY_MAX_LEVELS) return fail(nullptr, BHRAY_E_INVALID, "levels out of range");
    for (uint32_t i = 0; i < cfg->levels; i++)
        if (cfg->level_w[i] < 2 || cfg->level_h[i] < 2 || cfg->level_w[i] > 32767 || cfg->level_h[i] > 32767)
            return fail(nullptr, BHRAY_E_INVALID, "level %u size %ux%u unsupported", i, cfg->level_w[i], cfg->level_h[i]);
    const uint32_t lw = cfg->level_w[cfg->levels - 1], lh = cfg->level_h[cfg->levels - 1];
    if (cfg->frame_w < 1 || cfg->frame_h < 1 || cfg->crop_x + cfg->frame_w > lw || cfg->crop_y + cfg->frame_h > lh)
        return fail(nullptr, BHRAY_E_INVALID, "frame window outside the last level");
    if (cfg->row_world < 1 || cfg->row_rank >= cfg->row_world)
        return fail(nullptr, BHRAY_E_INVALID, "bad row partition");
    if (const char* why = partition_error(*cfg, cfg->row_world)) return fail(nullptr, BHRAY_E_INVALID, "bad row partition: %s", why);
    if (cfg->frames_in_flight > BHRAY_MAX_FRAMES_IN_FLIGHT) return fail(nullptr, BHRAY_E_INVALID, "frames_in_flight > %d", BHRAY_MAX_FRAMES_IN_FLIGHT);
    if (cfg->frames_per_batch > BHRAY_MAX_FRAMES_PER_BATCH) return fail(nullptr, BHRAY_E_INVALID, "frames_per_batch > %d", BHRAY_MAX_FRAMES_PER_BATCH);
    if (cfg->speculative_levels == 1 || cfg->speculative_levels > BHRAY_MAX_SPEC_LEVELS || (cfg->speculative_levels && cfg->speculative_levels >= cfg->levels))
        return fail(nullptr, BHRAY_E_INVALID, "speculative_levels must be 0 or 2..min(%d, levels-1)", BHRAY_MAX_SPEC_LEVELS);
    if (cfg->superset_levels == 1 || cfg->superset_levels > BHRAY_MAX_SPEC_LEVELS ||
        (cfg->superset_levels && cfg->superset_levels + (cfg->speculative_levels ? cfg->speculative_levels : 1) > cfg->levels))
        return fail(nullptr, BHRAY_E_INVALID, "superset_levels must be 0 or 2..%d and leave at least one coarser level (beyond the speculative ones)", BHRAY_MAX_SPEC_LEVELS);
    if ((cfg->flags & BHRAY_F_TEMPORAL) && (cfg->levels > BHRAY_MAX_SPEC_LEVELS || cfg->speculative_levels || cfg->superset_levels))
        return fail(nullptr, BHRAY_E_INVALID, "BHRAY_F_TEMPORAL needs levels <= %d and no speculative / superset levels", BHRAY_MAX_SPEC_LEVELS);
    if (cfg->flags & ~(uint32_t)BHRAY_F_ALL)
        return fail(nullptr, BHRAY_E_INVALID, "unknown bits in bhray_config.flags (0x%x; bit 6 was BHRAY_F_FUSED, the fused ladder of rounds 3-5: measured slower, removed - profiles/variants_src/)", cfg->flags & ~(uint32_t)BHRAY_F_ALL);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, BHRAY_E_NO_DEVICE, "no HIP device visible (libbhray has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, BHRAY_E_NO_DEVICE, "device %d not present (%d visible)", cfg->device, ndev);

    bhray_dev* c = new (std::nothrow) bhray_dev();
    if (!c) return fail(nullptr, BHRAY_E_NOMEM, "host allocation failed");
    c->cfg = *cfg;
    c->device = cfg->device;
    c->opt = opt;
#define CHK(call)                                                                                             \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            int rc_ = fail(nullptr, BHRAY_E_HIP, "%s: %s", #call, hipGetErrorString(e_));                     \
            dev_destroy(c);                                                                                 \
            return rc_;                                                                                       \
        }                                                                                                     \
    } while (0)
    CHK(hipSetDevice(c->device));
    hipDeviceProp_t prop;
    CHK(hipGetDeviceProperties(&prop, c->device));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char* e = getenv("BHRAY_TRACE_BLOCKS_PER_CU")) c->bpc_override = atoi(e);
    if (const char* e = getenv("BHRAY_TRACE_GRID")) c->grid_override = atoi(e);
    if (const char* e = getenv("BHRAY_PRIO")) c->wave_prio = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("BHRAY_QUAD")) { const int q = atoi(e); c->quad_wps = q < 0 ? 0 : (q > 4 ? 4 : q); }
    if (const char* e = getenv("BHRAY_TEMPORAL_MARGIN")) { const float m = (float)atof(e); c->temporal_margin = m < 0.05f ? 0.05f : (m > 1.0f ? 1.0f : m); }
    if (const char* e = getenv("BHRAY_TEMPORAL_RADIUS")) {          // "fine[,coarse]": the last level, the levels below it
        int rf = 0, rc = -1;
        const int n = sscanf(e, "%d,%d", &rf, &rc);
        if (n < 2) rc = rf;
        c->temporal_radius = rf < 0 ? 0 : (rf > 4 ? 4 : (uint32_t)rf);
        c->temporal_radius_coarse = rc < 0 ? 0 : (rc > 4 ? 4 : (uint32_t)rc);
    }
    if (const char* e = getenv("BHRAY_TRACE_DENSE")) c->dense_override = atoi(e) != 0;
    if (const char* e = getenv("BHRAY_COARSE_BUILD")) c->coarse_build = atoi(e);
    if (const char* e = getenv("BHRAY_ORIGIN_KERNEL")) c->origin_kernel = atoi(e) != 0;
    if (const char* e = getenv("BHRAY_DYNAMIC_DENSE")) c->dynamic_dense = atoi(e);
    if (const char* e = getenv("BHRAY_LEVEL_GRID")) c->level_grid = atoi(e) != 0;
    if (const char* e = getenv("BHRAY_LEVEL_GRID_GEN")) { const int v = atoi(e); if (v > 0) c->level_grid_gen = (uint32_t)v; }
    if (const char* e = getenv("BHRAY_LEVEL_GRID_MARGIN")) { const int v = atoi(e); if (v >= 0) c->level_grid_margin = (uint32_t)v; }
    if (const char* e = getenv("BHRAY_LEVEL_GRID_FLOOR")) { const int v = atoi(e); if (v >= 0) c->level_grid_floor = (uint32_t)v; }
    const uint32_t nslots = cfg->frames_in_flight ? cfg->frames_in_flight : 4;
    c->cfg.frames_in_flight = nslots;
    c->slots.resize(nslots);
    c->batch = cfg->frames_per_batch ? cfg->frames_per_batch : 1;
    c->cfg.frames_per_batch = c->batch;

    const uint32_t nl = cfg->levels;
    c->levels.resize(nl);
    for (uint32_t l = 0; l < nl; l++) { c->levels[l].w = (int)cfg->level_w[l]; c->levels[l].h = (int)cfg->level_h[l]; }
    for (uint32_t l = 0; l < nl; l++) c->row_work_off[l + 1] = c->row_work_off[l] + (size_t)cfg->level_h[l];
    // rows of the frame owned by this partition, the level rows they depend on, their device tables
    { int rc_ = build_row_tables(c); if (rc_) { g_create_error = c->err; dev_destroy(c); return rc_; } }
    // Argument blocks (FrameLaunch[B] each, BatchPlan::next_launch) a batch can need, by builder: speculative 2 ns (ns tentative classifies, the trace, ns - 1 classifies),
    // temporal 2 nl + 1 (nl predictions, the predicted trace, nl fix-up pairs that share a block), levels one per level, superset 2 nu + 1.  The modes a config can combine
    // (speculative + levels + superset; temporal alone) stay within 2 nl + 1; the worst BatchPlan::build could ever string together is speculative plus temporal,
    // 2 (nl - 1) + 2 nl + 1 < 4 nl + 1.  next_launch refuses the block that would not fit.
    const size_t nlaunch = 5 * (size_t)nl + 3;
    // Streams beyond the hardware queues ROCm maps them onto (GPU_MAX_HW_QUEUES, default 4; two are left to the null stream and a
    // communication stream) do not add concurrency, they alias - and a device with MORE streams than queues collapses (24 slots on 24
    // queues: 5 580 -> 4 380 Mrays/s, and a 20-frame block from 8.5 to 73 ms, measured).  The library only READS the variable: the slots
    // beyond the limit share the streams of the first ones (two frames on one stream are simply in order).
    size_t max_streams = 2;
    { const char* e = getenv("GPU_MAX_HW_QUEUES"); const int q = e ? atoi(e) : 4; max_streams = q > 3 ? (size_t)(q - 2) : 2; }
    if (opt.max_streams && max_streams > opt.max_streams) max_streams = opt.max_streams;
    for (size_t si = 0; si < c->slots.size(); si++) {
        Slot& S = c->slots[si];
        if (si < max_streams) CHK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
        else { S.stream = c->slots[si % max_streams].stream; S.owns_stream = false; }
        CHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
        CHK(hipEventCreateWithFlags(&S.uploaded, hipEventDisableTiming));
        const size_t B = c->batch;
        CHK(hipMalloc(&S.d_qctl, B * BHRAY_QCTL_WORDS * sizeof(uint32_t)));
        CHK(hipMemset(S.d_qctl, 0, B * BHRAY_QCTL_WORDS * sizeof(uint32_t)));
        CHK(hipMalloc(&S.d_counters, B * BHRAY_MAX_LEVELS * sizeof(Counters64)));
        CHK(hipMemset(S.d_counters, 0, B * BHRAY_MAX_LEVELS * sizeof(Counters64)));
        S.args_cap = (B * (sizeof(FrameParams) + nlaunch * sizeof(FrameLaunch) + 16) + 15) & ~(size_t)15;
        CHK(hipHostMalloc((void**)&S.h_args, S.args_cap, hipHostMallocDefault));
        CHK(hipMalloc(&S.d_args, S.args_cap));
        CHK(hipHostMalloc((void**)&S.h_qlen, B * BHRAY_LEVEL_GRID_LAUNCHES * sizeof(uint32_t), hipHostMallocDefault));
        for (size_t i = 0; i < B * BHRAY_LEVEL_GRID_LAUNCHES; i++) S.h_qlen[i] = QLEN_NONE;
        S.fr.resize(B);
        for (size_t k = 0; k < B; k++) {
            FrameRes& R = S.fr[k];
            R.d_qctl = S.d_qctl + k * BHRAY_QCTL_WORDS;
            R.d_work = reinterpret_cast<unsigned long long*>(R.d_qctl + 2 * BHRAY_MAX_LEVELS);
            R.d_counters = S.d_counters + k * BHRAY_MAX_LEVELS;
            R.level_out.assign(nl > 0 ? nl - 1 : 0, nullptr);
            R.queue.assign(nl, nullptr);
            for (uint32_t l = 0; l < nl; l++) {
                const Level& L = c->levels[l];
                if (l + 1 < nl) {
                    const size_t npix = (size_t)L.w * (size_t)L.h;
                    CHK(hipMalloc(&R.level_out[l], npix * sizeof(float4)));
                    CHK(hipMemset(R.level_out[l], 0xFF, npix * sizeof(float4)));      // NaN: "never rendered"
                }
            }
            if (cfg->speculative_levels) {
                const uint32_t ns = cfg->speculative_levels;
                R.spec_out.assign(ns, nullptr);
                for (uint32_t l = 0; l < ns; l++) {
                    const Level& L = c->levels[l];
                    if (l > 0) {
                        const size_t npix = (size_t)L.w * (size_t)L.h;
                        CHK(hipMalloc(&R.spec_out[l], npix * sizeof(float4)));
                        CHK(hipMemset(R.spec_out[l], 0xFF, npix * sizeof(float4)));
                    }
                }
            }
            if (cfg->flags & BHRAY_F_TEMPORAL) {
                R.stamp.assign(nl, nullptr); R.need.assign(nl, nullptr);
                for (uint32_t l = 0; l < nl; l++) {
                    const Level& L = c->levels[l];
                    const size_t npix = (size_t)L.w * (size_t)L.h;
                    CHK(hipMalloc(&R.stamp[l], npix * sizeof(uint32_t)));
                    CHK(hipMemset(R.stamp[l], 0, npix * sizeof(uint32_t)));
                    CHK(hipMalloc(&R.need[l], npix));
                    CHK(hipMemset(R.need[l], 0, npix));
                }
                static_assert(BHRAY_MAX_SPEC_LEVELS < BHRAY_MAX_LEVELS, "the predicted queue borrows the last level's control words");
                R.pred_ctl = R.d_qctl + 2 * (BHRAY_MAX_LEVELS - 1);
            }
            if (cfg->flags & BHRAY_F_COUNTERS) {
                CHK(hipMalloc(&R.d_row_work, c->row_work_off[nl] * sizeof(unsigned long long)));
                CHK(hipMemset(R.d_row_work, 0, c->row_work_off[nl] * sizeof(unsigned long long)));
            }
            R.out = R.own_out;
        }
    }
    // ray queues and own output buffers of every frame, sized for the partition (grown by dev_set_partition when it changes)
    { int rc_ = ensure_frame_buffers(c, false); if (rc_) { g_create_error = c->err; dev_destroy(c); return rc_; } }
    if (cfg->flags & (BHRAY_F_TIMING | BHRAY_F_TIMING_SPARSE)) {
        c->events.assign((size_t)BHRAY_TIMING_RING * events_per_batch(nl), nullptr);
        for (auto& e : c->events) CHK(hipEventCreate(&e));
        CHK(hipMalloc(&c->d_span, (size_t)BHRAY_TIMING_RING * SPAN_MAX * 2 * sizeof(unsigned long long)));
        CHK(hipMemset(c->d_span, 0, (size_t)BHRAY_TIMING_RING * SPAN_MAX * 2 * sizeof(unsigned long long)));
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) c->wall_clock_khz = (double)khz;
    }
    CHK(hipMalloc(&c->d_err, sizeof(int)));
    CHK(hipMemset(c->d_err, 0, sizeof(int)));
    // 1x1 opaque-black defaults so a missing texture cannot fault
    for (int s = 0; s < 3; s++) {
        const uint8_t px[4] = {0, 0, 0, 255};
        CHK(hipMalloc(&c->tex[s], 4));
        CHK(hipMemcpy(c->tex[s], px, 4, hipMemcpyHostToDevice));
        c->tex_w[s] = 1; c->tex_h[s] = 1;
    }
#undef CHK
    *out = c;
    return BHRAY_OK;
}

namespace {
// The pyramid of the resident sky texture, one launch per level on the legacy stream, complete on return.  Called with the engine idle (sync_all).
int build_sky_pyramid(bhray_dev* c) {
    if (c->pyr_buf) { (void)hipFree(c->pyr_buf); c->pyr_buf = nullptr; }
    c->pyr = SkyPyr{};
    if (!c->tex[BHRAY_TEX_SKY]) return BHRAY_OK;
    TexDev sky; sky.rgba = c->tex[BHRAY_TEX_SKY]; sky.w = c->tex_w[BHRAY_TEX_SKY]; sky.h = c->tex_h[BHRAY_TEX_SKY];
    SkyPyr P;
    const size_t texels = sky_pyramid_layout(sky.w, sky.h, &P);
    if (P.levels < 1) return fail(c, BHRAY_E_INVALID, "sky pyramid: bad texture size %d x %d", sky.w, sky.h);
    if (texels) {
        HIPCHK(c, hipMalloc(&c->pyr_buf, texels * sizeof(uint2)));
        HIPCHK(c, launch_sky_pyramid_first(sky, c->pyr_buf + P.off[1], nullptr));
        for (int l = 1; l + 1 < P.levels; l++)
            HIPCHK(c, launch_sky_pyramid_next(c->pyr_buf + P.off[l], sky_pyr_dim(sky.w, l), sky_pyr_dim(sky.h, l), c->pyr_buf + P.off[l + 1], nullptr));
        HIPCHK(c, hipStreamSynchronize(nullptr));
    }
    P.base = c->pyr_buf;
    c->pyr = P;
    return BHRAY_OK;
}
}  // namespace

int dev_set_texture(bhray_dev* c, int slot, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    if (!c) return BHRAY_E_INVALID;
    if (slot < 0 || slot > 2 || !rgba8 || w < 1 || h < 1 || w > 32768 || h > 32768) return fail(c, BHRAY_E_INVALID, "bad texture arguments");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }          // staged frames hold the old texture's address
    HIPCHK(c, sync_all(c));
    uint8_t* d = nullptr;
    const size_t bytes = (size_t)w * h * 4;
    HIPCHK(c, hipMalloc(&d, bytes));
    hipError_t e = hipMemcpy(d, rgba8, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return fail(c, BHRAY_E_HIP, "texture upload: %s", hipGetErrorString(e)); }
    if (c->tex[slot]) (void)hipFree(c->tex[slot]);
    c->tex[slot] = d; c->tex_w[slot] = (int)w; c->tex_h[slot] = (int)h;
    if (slot == BHRAY_TEX_SKY && c->sky_filter != 0) return build_sky_pyramid(c);
    return BHRAY_OK;
}

// The footprint-filtered sky pass: per-engine state, applied from the next dev_resolve_sky.  bhray_set_texture's rule: staged frames are launched
// and the frames in flight waited for, since a resolve enqueued under the other mode may still be reading the pyramid.
int dev_set_sky_filter(bhray_dev* c, int32_t mode) {
    if (!c) return BHRAY_E_INVALID;
    if (mode != 0 && mode != 1) return fail(c, BHRAY_E_INVALID, "bhray_set_sky_filter: mode %d (0: off, 1: footprint filter)", (int)mode);
    if (mode != 0 && (c->cfg.row_world > 1 || c->local_rows.size() != (size_t)c->cfg.frame_h))
        return fail(c, BHRAY_E_STATE, "bhray_set_sky_filter: not built for a row partition (a partition does not hold its neighbours' rows)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    HIPCHK(c, sync_all(c));
    c->sky_filter = mode;
    if (mode == 0) {
        if (c->pyr_buf) { (void)hipFree(c->pyr_buf); c->pyr_buf = nullptr; }
        c->pyr = SkyPyr{};
        return BHRAY_OK;
    }
    int rc = build_sky_pyramid(c);
    if (rc) c->sky_filter = 0;
    return rc;
}

// Point stars: per-engine state, applied from the next dev_resolve_sky.  bhray_set_texture's rule: staged frames are launched and the frames in
// flight waited for, since a resolve enqueued earlier may still be reading the old catalogue.  Everything that can refuse comes before anything is changed.
int dev_set_stars(bhray_dev* c, const bhray_star* stars, uint32_t n, const bhray_star_params* params) {
    if (!c) return BHRAY_E_INVALID;
    const bool on = stars != nullptr && n != 0;
    if (const char* why = stars_error(on ? stars : nullptr, on ? n : 0, params)) return fail(c, BHRAY_E_INVALID, "bhray_set_stars: %s", why);
    if (on && (c->cfg.row_world > 1 || c->local_rows.size() != (size_t)c->cfg.frame_h))
        return fail(c, BHRAY_E_STATE, "bhray_set_stars: not built for a row partition (a partition does not hold its neighbours' rows)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    HIPCHK(c, sync_all(c));
    float4* d_stars = nullptr; uint32_t* d_prefix = nullptr;
    StarSet S{};
    if (on) {
        bhray_star_params P;
        bhray_star_params_default(&P);
        if (params) P = *params;
        uint32_t G;
        std::vector<float4> sorted; std::vector<uint32_t> prefix;
        stars_build_index(stars, n, G, sorted, prefix);
        hipError_t e = hipMalloc(&d_stars, sorted.size() * sizeof(float4));
        if (e == hipSuccess) e = hipMalloc(&d_prefix, prefix.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(d_stars, sorted.data(), sorted.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_prefix, prefix.data(), prefix.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {                                       // the catalogue in force stays
            if (d_stars) (void)hipFree(d_stars);
            if (d_prefix) (void)hipFree(d_prefix);
            return fail(c, e == hipErrorOutOfMemory ? BHRAY_E_NOMEM : BHRAY_E_HIP, "bhray_set_stars: catalogue upload: %s", hipGetErrorString(e));
        }
        S = StarSet{d_stars, d_prefix, G, P.gain, P.min_area, P.max_footprint * P.max_footprint};
    }
    if (c->star_buf) (void)hipFree(c->star_buf);
    if (c->star_prefix) (void)hipFree(c->star_prefix);
    c->star_buf = d_stars; c->star_prefix = d_prefix; c->stars = S; c->star_count = on ? n : 0;
    return BHRAY_OK;
}

// bhray_diag.h: star_kernel with the engine's catalogue over a caller's frame.  Allocate, copy in, the product's launch_stars on the legacy stream, wait, copy out, free.
int dev_diag_star_image(bhray_dev* c, const float* frame, uint32_t w, uint32_t h, const uint16_t* sky_in, uint16_t* sky_out) {
    if (!c) return BHRAY_E_INVALID;
    if (!frame || !sky_out || w == 0 || h == 0 || w > 32767 || h > 32767) return fail(c, BHRAY_E_INVALID, "bhray_diag_star_image: NULL frame or output, or a frame that is empty or above 32767 pixels a side");
    if (!c->stars.stars) return fail(c, BHRAY_E_STATE, "bhray_diag_star_image: no catalogue (bhray_set_stars)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)w * h;
    float4* d_frame = nullptr; uint2* d_img = nullptr;
    const char* what = "hipMalloc";
    hipError_t e = hipMalloc(&d_frame, npix * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&d_img, npix * sizeof(uint2));
    if (e == hipSuccess) { what = "hipMemcpy"; e = hipMemcpy(d_frame, frame, npix * sizeof(float4), hipMemcpyHostToDevice); }
    if (e == hipSuccess) e = sky_in ? hipMemcpy(d_img, sky_in, npix * sizeof(uint2), hipMemcpyHostToDevice) : hipMemset(d_img, 0, npix * sizeof(uint2));
    if (e == hipSuccess) { what = "launch_stars"; e = launch_stars(c->stars, d_frame, d_img, w, h, nullptr); }
    if (e == hipSuccess) { what = "hipStreamSynchronize"; e = hipStreamSynchronize(nullptr); }
    if (e == hipSuccess) { what = "hipMemcpy"; e = hipMemcpy(sky_out, d_img, npix * sizeof(uint2), hipMemcpyDeviceToHost); }
    if (d_frame) (void)hipFree(d_frame);
    if (d_img) (void)hipFree(d_img);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? BHRAY_E_NOMEM : BHRAY_E_HIP, "bhray_diag_star_image: %s: %s", what, hipGetErrorString(e));
    return BHRAY_OK;
}

int dev_read_sky_pyramid_level(bhray_dev* c, uint32_t level, uint16_t* dst, size_t texels) {
    if (!c) return BHRAY_E_INVALID;
    if (c->sky_filter == 0 || !c->tex[BHRAY_TEX_SKY] || c->pyr.levels < 1) return fail(c, BHRAY_E_STATE, "bhray_read_sky_pyramid_level: the sky filter is off (bhray_set_sky_filter)");
    if (level == 0 || level >= (uint32_t)c->pyr.levels) return fail(c, BHRAY_E_INVALID, "bhray_read_sky_pyramid_level: level %u of a pyramid with levels 1 .. %d", level, c->pyr.levels - 1);
    const size_t n = (size_t)sky_pyr_dim(c->tex_w[BHRAY_TEX_SKY], (int)level) * (size_t)sky_pyr_dim(c->tex_h[BHRAY_TEX_SKY], (int)level);
    if (!dst || texels != n) return fail(c, BHRAY_E_INVALID, "bhray_read_sky_pyramid_level: level %u holds %zu texels", level, n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->pyr_buf + c->pyr.off[level], n * sizeof(uint2), hipMemcpyDeviceToHost));    // the pyramid was complete when its build returned
    return BHRAY_OK;
}

int dev_upload_model(bhray_dev* c, uint32_t mi, const bhray_model_desc* d) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS || !d) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    if (d->point_count < 0 || d->normal_count < 0 || d->triangle_count < 0 || d->node_count < 0 ||
        d->point_count > BHRAY_MAX_MODEL_VERTICES || d->normal_count > BHRAY_MAX_MODEL_VERTICES ||
        d->triangle_count > BHRAY_MAX_MODEL_VERTICES || d->node_count > BHRAY_MAX_MODEL_VERTICES)
        return fail(c, BHRAY_E_CAPACITY, "model exceeds MAX_MODEL_VERTICES (triangle.rs:7)");
    if (d->triangle_count > 0 && (!d->points || !d->normals || !d->triangles || !d->nodes || !d->bvh_lookup || d->node_count < 1))
        return fail(c, BHRAY_E_INVALID, "model arrays missing");
    // validate indices so the kernel never reads out of bounds
    for (int i = 0; i < d->triangle_count; i++) {
        const bhray_triangle& t = d->triangles[i];
        if (t.p1 < 0 || t.p2 < 0 || t.p3 < 0 || t.p1 >= d->point_count || t.p2 >= d->point_count || t.p3 >= d->point_count ||
            t.n1 < 0 || t.n2 < 0 || t.n3 < 0 || t.n1 >= d->normal_count || t.n2 >= d->normal_count || t.n3 >= d->normal_count)
            return fail(c, BHRAY_E_INVALID, "triangle %d has an index out of range", i);
        if (d->bvh_lookup[i] < 0 || d->bvh_lookup[i] >= d->triangle_count) return fail(c, BHRAY_E_INVALID, "bvh_lookup[%d] out of range", i);
    }
    for (int i = 0; i < d->node_count && d->triangle_count > 0; i++) {     // an empty model's root is (0 children, 0 objects): never traversed
        const bhray_node& n = d->nodes[i];
        if (n.obj_count < 0) return fail(c, BHRAY_E_INVALID, "node %d: negative obj_count", i);
        if (n.obj_count == 0) {
            if (n.left_child < 1 || n.left_child + 1 >= d->node_count)
                return fail(c, BHRAY_E_INVALID, "node %d: children out of range", i);
        } else if (n.left_child < 0 || (int64_t)n.left_child + n.obj_count > d->triangle_count) {
            return fail(c, BHRAY_E_INVALID, "node %d: leaf range out of bounds", i);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }          // staged frames hold the old model's addresses
    HIPCHK(c, sync_all(c));
    ModelStore& m = c->models[mi];
    free_model(m);
    memcpy(m.pos, d->position, 12);
    m.visible = d->visible;
    m.point_count = d->point_count; m.normal_count = d->normal_count; m.triangle_count = d->triangle_count; m.node_count = d->node_count;
    if (d->triangle_count > 0) {
        HIPCHK(c, hipMalloc(&m.points, (size_t)d->point_count * 16));
        HIPCHK(c, hipMalloc(&m.normals, (size_t)d->normal_count * 16));
        HIPCHK(c, hipMalloc(&m.triangles, (size_t)d->triangle_count * 24));
        HIPCHK(c, hipMalloc(&m.nodes, (size_t)d->node_count * 32));
        HIPCHK(c, hipMalloc(&m.lookup, (size_t)d->triangle_count * 4));
        HIPCHK(c, hipMemcpy(m.points, d->points, (size_t)d->point_count * 16, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(m.normals, d->normals, (size_t)d->normal_count * 16, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(m.triangles, d->triangles, (size_t)d->triangle_count * 24, hipMemcpyHostToDevice));
        // Nodes are re-numbered breadth-first for the device (the builder numbers them depth-first, triangle.rs:239-258):
        // the top of the tree, which every traversal touches, is then contiguous (cache locality).  Children stay adjacent
        // and leaf ranges are untouched, so traversal order and results do not change.
        {
            std::vector<bhray_node> bfs((size_t)d->node_count);
            std::vector<int32_t> order; order.reserve((size_t)d->node_count);
            order.push_back(0);
            size_t next = 1;
            for (size_t q = 0; q < order.size(); q++) {
                const bhray_node& n = d->nodes[(size_t)order[q]];
                bfs[q] = n;
                if (n.obj_count == 0) {
                    if (next + 2 > (size_t)d->node_count) return fail(c, BHRAY_E_INVALID, "malformed BVH (unreachable or shared nodes)");
                    bfs[q].left_child = (int32_t)next;
                    order.push_back(n.left_child); order.push_back(n.left_child + 1);
                    next += 2;
                }
            }
            m.node_count = (int)order.size();
            // what the traversal's first visit tests: the two children of the (untested) root.  A ray that misses the union
            // of their boxes misses both (the slab test is monotone in the box), so the kernel can skip that visit.
            if (bfs[0].obj_count == 0 && order.size() >= 3) {
                for (int a = 0; a < 3; a++) {
                    m.root_lo[a] = bfs[1].min_corner[a] < bfs[2].min_corner[a] ? bfs[1].min_corner[a] : bfs[2].min_corner[a];
                    m.root_hi[a] = bfs[1].max_corner[a] > bfs[2].max_corner[a] ? bfs[1].max_corner[a] : bfs[2].max_corner[a];
                }
                bool finite = true;
                for (int a = 0; a < 3; a++) finite = finite && std::isfinite(m.root_lo[a]) && std::isfinite(m.root_hi[a]);
                m.root_cull = finite ? 1 : 0;
            }
            HIPCHK(c, hipMemcpy(m.nodes, bfs.data(), order.size() * 32, hipMemcpyHostToDevice));
        }
        HIPCHK(c, hipMemcpy(m.lookup, d->bvh_lookup, (size_t)d->triangle_count * 4, hipMemcpyHostToDevice));
        // pre-gathered leaf geometry: slot k holds the points and normals of triangle bvh_lookup[k] (copies, same bits)
        {
            std::vector<float> leaf((size_t)d->triangle_count * 24);
            for (int k = 0; k < d->triangle_count; k++) {
                const bhray_triangle& t = d->triangles[d->bvh_lookup[k]];
                const int32_t pi[3] = {t.p1, t.p2, t.p3}, ni[3] = {t.n1, t.n2, t.n3};
                for (int v = 0; v < 3; v++) {
                    memcpy(&leaf[(size_t)k * 24 + 4 * v], d->points + 4 * (size_t)pi[v], 16);
                    memcpy(&leaf[(size_t)k * 24 + 12 + 4 * v], d->normals + 4 * (size_t)ni[v], 16);
                }
            }
            HIPCHK(c, hipMalloc(&m.leaf, leaf.size() * 4));
            HIPCHK(c, hipMemcpy(m.leaf, leaf.data(), leaf.size() * 4, hipMemcpyHostToDevice));
        }
    }
    m.loaded = true;
    return BHRAY_OK;
}

namespace {
// The build of slot `m` from the points, normals and triangles it holds, on the engine's first stream, timed; then the 64 bytes of result.
// `copies` enqueues the host-to-device copies of this call between the first two events.
template <class Copies>
int build_on_device(bhray_dev* c, ModelStore& m, Copies copies) {
    hipStream_t s = c->slots[0].stream;
    HIPCHK(c, hipEventRecord(m.ev[0], s));
    { int rc = copies(s); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(m.ev[1], s));
    HIPCHK(c, launch_bvh_build(m.build, m.points, m.normals, m.triangles, m.nodes, m.lookup, m.leaf, m.d_result, s));
    HIPCHK(c, hipEventRecord(m.ev[2], s));
    BvhResult r;
    HIPCHK(c, hipMemcpyAsync(&r, m.d_result, sizeof r, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (r.max_depth == 0 || r.max_depth > BHRAY_LBVH_MAX_PASSES || r.nodes < 1 || r.nodes > 2u * (uint32_t)m.triangle_count - 1u)
        return fail(c, BHRAY_E_BVH_DEPTH, "device BVH build: the box passes did not reach the root (%u nodes, depth %u)", r.nodes, r.max_depth);
    m.node_count = (int)r.nodes;
    m.root_cull = r.root_cull; memcpy(m.root_lo, r.root_lo, 12); memcpy(m.root_hi, r.root_hi, 12);
    m.info.built_on_device = 1; m.info.triangles = (uint32_t)m.triangle_count; m.info.nodes = r.nodes; m.info.leaves = r.leaves;
    m.info.max_leaf = r.max_leaf; m.info.max_depth = r.max_depth;
    HIPCHK(c, hipEventElapsedTime(&m.info.upload_ms, m.ev[0], m.ev[1]));
    HIPCHK(c, hipEventElapsedTime(&m.info.build_ms, m.ev[1], m.ev[2]));
    return BHRAY_OK;
}
}  // namespace

int dev_upload_model_build(bhray_dev* c, uint32_t mi, const bhray_model_desc* d) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS || !d) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    if (d->point_count < 0 || d->normal_count < 0 || d->triangle_count < 0 || d->point_count > BHRAY_MAX_MODEL_VERTICES ||
        d->normal_count > BHRAY_MAX_MODEL_VERTICES || d->triangle_count > BHRAY_MAX_MODEL_VERTICES)
        return fail(c, BHRAY_E_CAPACITY, "model exceeds MAX_MODEL_VERTICES (triangle.rs:7)");
    if (d->triangle_count > 0 && (!d->points || !d->normals || !d->triangles)) return fail(c, BHRAY_E_INVALID, "model arrays missing");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }          // staged frames hold the old model's addresses
    HIPCHK(c, sync_all(c));
    ModelStore n;                                             // built beside the slot: a refused model leaves the slot as it was
    memcpy(n.pos, d->position, 12);
    n.visible = d->visible;
    n.point_count = d->point_count; n.normal_count = d->normal_count; n.triangle_count = d->triangle_count;
    n.info.triangles = (uint32_t)d->triangle_count;
    if (d->triangle_count > 0) {
        const size_t T = (size_t)d->triangle_count;
        hipStream_t s = c->slots[0].stream;
        int rc = BHRAY_OK, bad = 0;
        auto hip = [&](hipError_t e, const char* what) { if (rc == BHRAY_OK && e != hipSuccess) rc = fail(c, BHRAY_E_HIP, "%s: %s", what, hipGetErrorString(e)); return rc == BHRAY_OK; };
        // index 0 of an empty points / normals array cannot be valid; one element keeps the allocations non-empty
        hip(hipMalloc(&n.points, (size_t)std::max(d->point_count, 1) * 16), "hipMalloc(points)") && hip(hipMalloc(&n.normals, (size_t)std::max(d->normal_count, 1) * 16), "hipMalloc(normals)") &&
            hip(hipMalloc(&n.triangles, T * 24), "hipMalloc(triangles)") && hip(hipMalloc(&n.nodes, (2 * T - 1) * 32), "hipMalloc(nodes)") &&
            hip(hipMalloc(&n.lookup, T * 4), "hipMalloc(lookup)") && hip(hipMalloc(&n.leaf, T * 96), "hipMalloc(leaf)") &&
            hip(hipMalloc(&n.d_result, sizeof(BvhResult)), "hipMalloc(result)") && hip(bvh_build_create(d->triangle_count, &n.build), "device BVH scratch");
        for (hipEvent_t& e : n.ev) if (rc == BHRAY_OK) hip(hipEventCreate(&e), "hipEventCreate");
        if (rc == BHRAY_OK) hip(hipMemcpyAsync(n.triangles, d->triangles, T * 24, hipMemcpyHostToDevice, s), "triangle upload");
        if (rc == BHRAY_OK) hip(launch_bvh_validate(n.build, n.triangles, d->point_count, d->normal_count, &bad, s), "index validation");
        if (rc == BHRAY_OK && bad != 0) rc = fail(c, BHRAY_E_INVALID, "a triangle has an index out of range");
        if (rc == BHRAY_OK)
            rc = build_on_device(c, n, [&](hipStream_t st) {
                HIPCHK(c, hipMemcpyAsync(n.points, d->points, (size_t)d->point_count * 16, hipMemcpyHostToDevice, st));
                HIPCHK(c, hipMemcpyAsync(n.normals, d->normals, (size_t)d->normal_count * 16, hipMemcpyHostToDevice, st));
                return (int)BHRAY_OK;
            });
        if (rc != BHRAY_OK) { std::string keep = c->err; (void)hipStreamSynchronize(s); free_model(n); c->err = keep; return rc; }
    }
    n.loaded = true;
    free_model(c->models[mi]);
    c->models[mi] = n;
    return BHRAY_OK;
}

namespace {
// bhray_update_model_vertices (kind = hipMemcpyHostToDevice) and bhray_update_model_vertices_device (hipMemcpyDefault, behind `after`).  On a posed slot the new
// arrays are the new REST arrays and the pose in force is applied again; on any other slot they are what the build reads.
int update_vertices(bhray_dev* c, uint32_t mi, const void* points, int32_t point_count, const void* normals, int32_t normal_count, hipMemcpyKind kind, hipEvent_t after, const char* name) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    ModelStore& m = c->models[mi];
    if (!m.loaded || !m.build) return fail(c, BHRAY_E_STATE, "%s: slot %u was not built by bhray_upload_model_build", name, mi);
    if ((points && point_count != m.point_count) || (normals && normal_count != m.normal_count))
        return fail(c, BHRAY_E_INVALID, "%s: the slot holds %d points and %d normals", name, m.point_count, m.normal_count);
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }          // staged frames show the old geometry
    HIPCHK(c, sync_all(c));                                   // and the frames in flight read the buffers that are rewritten here
    if (after) HIPCHK(c, hipStreamWaitEvent(c->slots[0].stream, after, 0));
    return build_on_device(c, m, [&](hipStream_t st) {
        if (points) HIPCHK(c, hipMemcpyAsync(m.posed ? m.rest_points : m.points, points, (size_t)m.point_count * 16, kind, st));
        if (normals) HIPCHK(c, hipMemcpyAsync(m.posed ? m.rest_normals : m.normals, normals, (size_t)m.normal_count * 16, kind, st));
        if (m.posed) HIPCHK(c, launch_bvh_pose(m.rest_points, m.rest_normals, m.points, m.normals, m.point_count, m.normal_count, m.pose, st));
        return (int)BHRAY_OK;
    });
}
}  // namespace

int dev_update_model_vertices(bhray_dev* c, uint32_t mi, const float* points, int32_t point_count, const float* normals, int32_t normal_count) {
    return update_vertices(c, mi, points, point_count, normals, normal_count, hipMemcpyHostToDevice, nullptr, "bhray_update_model_vertices");
}

int dev_update_model_vertices_device(bhray_dev* c, uint32_t mi, const void* d_points, int32_t point_count, const void* d_normals, int32_t normal_count, hipEvent_t after) {
    return update_vertices(c, mi, d_points, point_count, d_normals, normal_count, hipMemcpyDefault, after, "bhray_update_model_vertices_device");
}

// DESIGN.md §14.  The pose is absolute: always rest arrays -> points / normals.  NULL: the rest arrays back, byte for byte.
int dev_set_model_pose(bhray_dev* c, uint32_t mi, const float* pose) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    ModelStore& m = c->models[mi];
    if (!m.loaded || !m.build) return fail(c, BHRAY_E_STATE, "bhray_set_model_pose: slot %u was not built by bhray_upload_model_build", mi);
    if (pose) for (int i = 0; i < 12; i++) if (!std::isfinite(pose[i])) return fail(c, BHRAY_E_INVALID, "bhray_set_model_pose: pose entry %d is not finite", i);
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }          // staged frames show the old geometry
    HIPCHK(c, sync_all(c));
    hipStream_t s = c->slots[0].stream;
    const size_t pb = (size_t)std::max(m.point_count, 1) * 16, nb = (size_t)std::max(m.normal_count, 1) * 16;
    if (pose && !m.posed) {                                   // what the slot holds now is its rest geometry
        if (!m.rest_points) HIPCHK(c, hipMalloc(&m.rest_points, pb));
        if (!m.rest_normals) HIPCHK(c, hipMalloc(&m.rest_normals, nb));
        HIPCHK(c, hipMemcpyAsync(m.rest_points, m.points, (size_t)m.point_count * 16, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(m.rest_normals, m.normals, (size_t)m.normal_count * 16, hipMemcpyDeviceToDevice, s));
    }
    const bool restore = !pose && m.posed;
    if (pose) { memcpy(m.pose, pose, sizeof m.pose); m.posed = true; } else m.posed = false;
    return build_on_device(c, m, [&](hipStream_t st) {
        if (m.posed) HIPCHK(c, launch_bvh_pose(m.rest_points, m.rest_normals, m.points, m.normals, m.point_count, m.normal_count, m.pose, st));
        else if (restore) {
            HIPCHK(c, hipMemcpyAsync(m.points, m.rest_points, (size_t)m.point_count * 16, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(m.normals, m.rest_normals, (size_t)m.normal_count * 16, hipMemcpyDeviceToDevice, st));
        }
        return (int)BHRAY_OK;
    });
}

int dev_get_model_build_info(bhray_dev* c, uint32_t mi, bhray_model_build_info* out) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS || !out) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    const ModelStore& m = c->models[mi];
    if (!m.loaded) return fail(c, BHRAY_E_STATE, "model slot %u is empty", mi);
    *out = m.info;
    out->triangles = (uint32_t)m.triangle_count; out->nodes = (uint32_t)m.node_count;
    return BHRAY_OK;
}

int dev_read_model_bvh(bhray_dev* c, uint32_t mi, bhray_node* nodes, uint32_t node_cap, int32_t* lookup, uint32_t lookup_cap, uint32_t* node_count, uint32_t* triangle_count) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    const ModelStore& m = c->models[mi];
    if (!m.loaded) return fail(c, BHRAY_E_STATE, "model slot %u is empty", mi);
    const uint32_t nn = m.triangle_count > 0 ? (uint32_t)m.node_count : 0u, nt = (uint32_t)m.triangle_count;
    if (node_count) *node_count = nn;
    if (triangle_count) *triangle_count = nt;
    if (nn > node_cap || nt > lookup_cap || (nn > 0 && !nodes) || (nt > 0 && !lookup)) return fail(c, BHRAY_E_INVALID, "bhray_read_model_bvh: the slot holds %u nodes and %u triangles", nn, nt);
    HIPCHK(c, hipSetDevice(c->device));
    if (nn > 0) HIPCHK(c, hipMemcpy(nodes, m.nodes, (size_t)nn * 32, hipMemcpyDeviceToHost));
    if (nt > 0) HIPCHK(c, hipMemcpy(lookup, m.lookup, (size_t)nt * 4, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

int dev_read_model_vertices(bhray_dev* c, uint32_t mi, float* points, uint32_t point_cap, float* normals, uint32_t normal_cap, uint32_t* point_count, uint32_t* normal_count) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    const ModelStore& m = c->models[mi];
    if (!m.loaded) return fail(c, BHRAY_E_STATE, "model slot %u is empty", mi);
    const uint32_t np = m.triangle_count > 0 ? (uint32_t)m.point_count : 0u, nn = m.triangle_count > 0 ? (uint32_t)m.normal_count : 0u;   // a slot of 0 triangles holds no arrays
    if (point_count) *point_count = np;
    if (normal_count) *normal_count = nn;
    if ((points && np > point_cap) || (normals && nn > normal_cap)) return fail(c, BHRAY_E_INVALID, "bhray_read_model_vertices: the slot holds %u points and %u normals", np, nn);
    HIPCHK(c, hipSetDevice(c->device));
    if (points && np > 0) HIPCHK(c, hipMemcpy(points, m.points, (size_t)np * 16, hipMemcpyDeviceToHost));
    if (normals && nn > 0) HIPCHK(c, hipMemcpy(normals, m.normals, (size_t)nn * 16, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

int dev_upload_model_uniform(bhray_dev* c, uint32_t mi, const void* bytes, size_t size) {
    if (!c) return BHRAY_E_INVALID;
    if (!bytes || size != BHRAY_MODEL_UNIFORM_BYTES) return fail(c, BHRAY_E_INVALID, "ModelUniform must be %u bytes", BHRAY_MODEL_UNIFORM_BYTES);
    const uint8_t* b = (const uint8_t*)bytes;
    bhray_model_header hd; memcpy(&hd, b, sizeof hd);
    bhray_model_desc d; memset(&d, 0, sizeof d);
    memcpy(d.position, hd.position, 12); d.visible = hd.visible;
    d.points = (const float*)(b + BHRAY_MODEL_OFF_POINTS);
    d.normals = (const float*)(b + BHRAY_MODEL_OFF_NORMALS);
    d.triangles = (const bhray_triangle*)(b + BHRAY_MODEL_OFF_TRIANGLES);
    d.nodes = (const bhray_node*)(b + BHRAY_MODEL_OFF_NODES);
    d.bvh_lookup = (const int32_t*)(b + BHRAY_MODEL_OFF_LOOKUP);
    d.point_count = hd.point_count; d.triangle_count = hd.triangle_count;
    if (d.triangle_count < 0 || d.triangle_count > BHRAY_MAX_MODEL_VERTICES || d.point_count < 0 || d.point_count > BHRAY_MAX_MODEL_VERTICES)
        return fail(c, BHRAY_E_CAPACITY, "counts in ModelUniform header out of range");
    // ModelUniform::update never copies normal_count (triangle.rs:308-325) and carries no node
    // count: recover both from the index data.
    int nmax = -1;
    for (int i = 0; i < d.triangle_count; i++) {
        const bhray_triangle& t = d.triangles[i];
        nmax = t.n1 > nmax ? t.n1 : nmax; nmax = t.n2 > nmax ? t.n2 : nmax; nmax = t.n3 > nmax ? t.n3 : nmax;
    }
    if (nmax >= BHRAY_MAX_MODEL_VERTICES) return fail(c, BHRAY_E_INVALID, "normal index out of range");
    d.normal_count = nmax + 1;
    int node_max = 0;
    if (d.triangle_count > 0) {
        std::vector<int> st; st.push_back(0);
        size_t visited = 0;
        while (!st.empty()) {
            int n = st.back(); st.pop_back();
            if (n < 0 || n >= BHRAY_MAX_MODEL_VERTICES || ++visited > (size_t)BHRAY_MAX_MODEL_VERTICES) return fail(c, BHRAY_E_INVALID, "malformed BVH");
            node_max = n > node_max ? n : node_max;
            if (d.nodes[n].obj_count == 0) { st.push_back(d.nodes[n].left_child); st.push_back(d.nodes[n].left_child + 1); }
        }
    }
    d.node_count = d.triangle_count > 0 ? node_max + 1 : 0;
    return dev_upload_model(c, mi, &d);
}

int dev_set_model_transform(bhray_dev* c, uint32_t mi, const float position[3], int32_t visible) {
    if (!c) return BHRAY_E_INVALID;
    if (mi >= BHRAY_MAX_MODELS || !position) return fail(c, BHRAY_E_INVALID, "bad model arguments");
    memcpy(c->models[mi].pos, position, 12);
    c->models[mi].visible = visible;
    return BHRAY_OK;
}

// Per-frame state like the uniforms: applies from the next dev_render; frames staged for the other kernel variant are launched first, there (a batch is homogeneous).
int dev_set_mesh_lensing(bhray_dev* c, int32_t on) {
    if (!c) return BHRAY_E_INVALID;
    if (on != 0 && (c->cfg.flags & (BHRAY_F_LITERAL | BHRAY_F_EVAL_FMA)))
        return fail(c, BHRAY_E_STATE, "mesh lensing has no kernel for BHRAY_F_LITERAL / BHRAY_F_EVAL_FMA (no executed shader text to pin one against)");
    c->mesh_lensing = on != 0;                                    // frames: any non-zero word (BHRAY_LENS_FRAMES is what `on != 0` has always meant)
    c->lens_rays = (on & BHRAY_LENS_RAYS) != 0;
    return BHRAY_OK;
}

int dev_set_uniforms(bhray_dev* c, const void* cam32, const void* bh132, const void* det32) {
    if (!c) return BHRAY_E_INVALID;
    if (!cam32 || !bh132 || !det32) return fail(c, BHRAY_E_INVALID, "null uniform block");
    static_assert(sizeof(bhray_camera_uniform) == 32 && sizeof(bhray_black_hole_uniform) == 132 && sizeof(bhray_details) == 32, "layout");
    memcpy(&c->cam, cam32, 32); memcpy(&c->bh, bh132, 132); memcpy(&c->det, det32, 32);
    c->have_uniforms = true;
    return BHRAY_OK;
}

// ---- ray batches (include/bhray.h: bhray_trace_rays) ------------------------------------------------------------
namespace {
constexpr size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
constexpr size_t Q_OFF_LAUNCH = align16(sizeof(FrameParams)), Q_OFF_CTL = Q_OFF_LAUNCH + align16(sizeof(FrameLaunch)), Q_ARGS_BYTES = Q_OFF_CTL + 16;

// why this engine traces no ray batch now (the refused states), or BHRAY_OK.  Under mesh lensing a batch needs the setting's BHRAY_LENS_RAYS bit, and a path
// call (path_call) is refused with either bit: there is no lensed path kernel
int rays_refused(bhray_dev* c, const char* name, bool path_call = false) {
    if (!c->have_uniforms) return fail(c, BHRAY_E_STATE, "%s: bhray_set_uniforms has not been called", name);
    if (c->cfg.flags & (BHRAY_F_LITERAL | BHRAY_F_EVAL_FMA)) return fail(c, BHRAY_E_STATE, "%s: no ray-list kernel for BHRAY_F_LITERAL / BHRAY_F_EVAL_FMA", name);
    if (c->mesh_lensing && (!c->lens_rays || path_call)) return fail(c, BHRAY_E_STATE, "%s: ray batches under mesh lensing are not built", name);
    return BHRAY_OK;
}

int ensure_query(bhray_dev* c) {
    if (!c->q_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->q_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&c->q_begin, &c->q_done, &c->q_uploaded}) if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (!c->q_hargs) HIPCHK(c, hipHostMalloc(&c->q_hargs, Q_ARGS_BYTES));
    if (!c->q_dargs) HIPCHK(c, hipMalloc(&c->q_dargs, Q_ARGS_BYTES));
    return BHRAY_OK;
}

// One launch on the query stream: n rays at d_rays -> n results at d_out, under the engine's current uniforms, textures and models.  Enqueues only.
// d_records: nullptr, or n bhray_ray_record (16-byte aligned) - the record kernels (TraceVariant::records).
// paths: nullptr, or the path arguments (d_records is then not null) - the path kernels (TraceVariant::paths).
struct PathArgs { void* d_points; void* d_counts; uint32_t stride_log2, max_points; };
int enqueue_rays(bhray_dev* c, const float4* d_rays, uint32_t n, float4* d_out, void* d_records = nullptr, const PathArgs* paths = nullptr) {
    // the pinned block of the batch before must have reached the device before it is rewritten (its device copy is read in stream order)
    if (c->q_used && hipEventQuery(c->q_uploaded) != hipSuccess) HIPCHK(c, hipEventSynchronize(c->q_uploaded));
    FrameParams& P = *(FrameParams*)c->q_hargs;
    derive_frame(c, P);                                           // exactly a frame's; the ray-list kernels read none of the camera members
    FrameLaunch& F = *(FrameLaunch*)(c->q_hargs + Q_OFF_LAUNCH);
    memset(&F, 0, sizeof F);
    F.L.w = (int)n; F.L.h = 1;
    F.L.prev = d_rays; F.L.out = d_out;                           // the records and the results (TraceVariant::rays)
    F.qctl = (uint32_t*)(c->q_dargs + Q_OFF_CTL);                 // [0] = n, [1] = 0: uploaded with the block, so the launch needs no reset of its own
    uint32_t* ctl = (uint32_t*)(c->q_hargs + Q_OFF_CTL);
    ctl[0] = n; ctl[1] = 0; ctl[2] = 0; ctl[3] = 0;
    F.row_work = (unsigned long long*)d_records;                  // the records (TraceVariant::records): the member a ray-list launch does not use otherwise
    if (paths) {                                                  // the paths (TraceVariant::paths): members of the classification and of temporal speculation, which no ray-list launch reads
        F.need = (uint8_t*)paths->d_points; F.stamp = (const uint32_t*)paths->d_counts;
        F.radius = (int)paths->stride_log2; F.stamp_value = paths->max_points;
    }
    // models: as a frame's (frame_variant) - lensed when the setting in force has BHRAY_LENS_RAYS and a usable visible model exists; the entry points refuse paths under lensing
    const TraceVariant v{P.method, P.model_count > 0 ? ((c->mesh_lensing && c->lens_rays && !paths) ? 2 : 1) : 0, false, false, 0, false, true, d_records != nullptr, paths != nullptr};
    int ctx_grid = c->num_cus * trace_blocks_per_cu(v);
    if (c->grid_override > 0) ctx_grid = c->grid_override;
    const int grid = (int)bhray_trace_grid_for(n, 1, (uint32_t)ctx_grid, c->level_grid_gen, 0, c->level_grid_floor);      // n is exact: no margin
    HIPCHK(c, launch_upload(c->q_hargs, c->q_dargs, Q_ARGS_BYTES / 16, nullptr, 0, c->q_stream));
    HIPCHK(c, hipEventRecord(c->q_uploaded, c->q_stream));
    c->q_used = true;
    HIPCHK(c, launch_trace((const FrameParams*)c->q_dargs, (const FrameLaunch*)(c->q_dargs + Q_OFF_LAUNCH), 1, v, c->d_err, grid, c->q_stream));
    return BHRAY_OK;
}
}  // namespace

// out: n x RGBA32F (may be NULL when sky16 is not); sky16: NULL, or n x RGBA16F - sky.wgsl over the results (launch_sky, the pass of dev_resolve_sky)
// records: NULL, or n records (bhray_trace_rays_records: then `out` may be NULL too)
// paths: NULL, or the path outputs (bhray_trace_rays_paths, whose entry has checked them: then `out` and `records` may be NULL) - n * max_points points, n counts
int dev_trace_rays(bhray_dev* c, const bhray_ray* rays, uint32_t n, float* out, uint16_t* sky16, bhray_ray_record* records, const bhray_dev_paths* paths) {
    if (!c) return BHRAY_E_INVALID;
    if (n > BHRAY_MAX_RAYS_PER_CALL || (n != 0 && (!rays || (!out && !sky16 && !records && !paths)))) return fail(c, BHRAY_E_INVALID, "bhray_trace_rays: bad arguments");
    if (paths && (paths->max_points < 2u || paths->stride_log2 > BHRAY_MAX_PATH_STRIDE_LOG2 || (uint64_t)n * paths->max_points > BHRAY_MAX_PATH_POINTS_PER_CALL ||
                  (n != 0 && (!paths->points || !paths->counts)))) return fail(c, BHRAY_E_INVALID, "bhray_trace_rays_paths: bad arguments");
    { int rc = rays_refused(c, "bhray_trace_rays", paths != nullptr); if (rc) return rc; }
    if (n == 0) return BHRAY_OK;
    for (uint32_t i = 0; i < n; i++) {                            // before anything is enqueued
        const float* o = rays[i].origin; const float* d = rays[i].direction;
        const bool finite = std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]) && std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]);
        if (!finite || (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f))
            return fail(c, BHRAY_E_INVALID, "bhray_trace_rays: ray %u has a non-finite component or a zero direction", i);
    }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }              // the staged frames first: they keep the uniforms they were staged with
    { int rc = ensure_query(c); if (rc) return rc; }
    if (n > c->q_cap) {                                           // grow-only staging
        HIPCHK(c, hipStreamSynchronize(c->q_stream));
        if (c->q_hin) (void)hipHostFree(c->q_hin);
        if (c->q_hout) (void)hipHostFree(c->q_hout);
        if (c->q_din) (void)hipFree(c->q_din);
        if (c->q_dout) (void)hipFree(c->q_dout);
        c->q_hin = c->q_hout = c->q_din = c->q_dout = nullptr; c->q_cap = 0;
        const size_t cap = std::max<size_t>(n, 4096);
        HIPCHK(c, hipHostMalloc(&c->q_hin, cap * sizeof(bhray_ray)));
        HIPCHK(c, hipHostMalloc(&c->q_hout, cap * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->q_din, cap * sizeof(bhray_ray)));
        HIPCHK(c, hipMalloc(&c->q_dout, cap * sizeof(float4)));
        c->q_cap = cap;
    } else {
        HIPCHK(c, hipStreamSynchronize(c->q_stream));           // (a copy of an earlier call that failed half-way may still read the staging)
    }
    const bool want_rec = records || paths;                       // the path kernels are record kernels: their records are staged whether the caller takes them or not
    const size_t npts = paths ? (size_t)n * paths->max_points : 0;
    if (paths && npts > c->q_pts_cap) {                           // the same for the points and the counts (the stream is idle here)
        if (c->q_hpts) (void)hipHostFree(c->q_hpts);
        if (c->q_dpts) (void)hipFree(c->q_dpts);
        c->q_hpts = c->q_dpts = nullptr; c->q_pts_cap = 0;
        const size_t cap = std::max<size_t>(npts, 65536);
        HIPCHK(c, hipHostMalloc(&c->q_hpts, cap * sizeof(bhray_path_point)));
        HIPCHK(c, hipMalloc(&c->q_dpts, cap * sizeof(bhray_path_point)));
        c->q_pts_cap = cap;
    }
    if (paths && n > c->q_cnt_cap) {
        if (c->q_hcnt) (void)hipHostFree(c->q_hcnt);
        if (c->q_dcnt) (void)hipFree(c->q_dcnt);
        c->q_hcnt = c->q_dcnt = nullptr; c->q_cnt_cap = 0;
        const size_t cap = std::max<size_t>(n, 4096);
        HIPCHK(c, hipHostMalloc(&c->q_hcnt, cap * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc(&c->q_dcnt, cap * sizeof(uint32_t)));
        c->q_cnt_cap = cap;
    }
    if (want_rec && n > c->q_rec_cap) {                           // the same for the records (the stream is idle here)
        if (c->q_hrec) (void)hipHostFree(c->q_hrec);
        if (c->q_drec) (void)hipFree(c->q_drec);
        c->q_hrec = c->q_drec = nullptr; c->q_rec_cap = 0;
        const size_t cap = std::max<size_t>(n, 4096);
        HIPCHK(c, hipHostMalloc(&c->q_hrec, cap * sizeof(bhray_ray_record)));
        HIPCHK(c, hipMalloc(&c->q_drec, cap * sizeof(bhray_ray_record)));
        c->q_rec_cap = cap;
    }
    memcpy(c->q_hin, rays, (size_t)n * sizeof(bhray_ray));
    HIPCHK(c, hipMemcpyAsync(c->q_din, c->q_hin, (size_t)n * sizeof(bhray_ray), hipMemcpyHostToDevice, c->q_stream));
    PathArgs pa{};
    if (paths) {                                                  // slots the kernel does not write come back as zero bytes
        pa = PathArgs{c->q_dpts, c->q_dcnt, paths->stride_log2, paths->max_points};
        HIPCHK(c, hipMemsetAsync(c->q_dpts, 0, npts * sizeof(bhray_path_point), c->q_stream));
    }
    { int rc = enqueue_rays(c, c->q_din, n, c->q_dout, want_rec ? c->q_drec : nullptr, paths ? &pa : nullptr); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(c->q_hout, c->q_dout, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->q_stream));
    if (records) HIPCHK(c, hipMemcpyAsync(c->q_hrec, c->q_drec, (size_t)n * sizeof(bhray_ray_record), hipMemcpyDeviceToHost, c->q_stream));
    if (paths) {
        HIPCHK(c, hipMemcpyAsync(c->q_hpts, c->q_dpts, npts * sizeof(bhray_path_point), hipMemcpyDeviceToHost, c->q_stream));
        HIPCHK(c, hipMemcpyAsync(c->q_hcnt, c->q_dcnt, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->q_stream));
    }
    if (sky16) {                                                  // the records are used up: their device buffer (32 bytes per ray) takes the image (8), their pinned one its copy
        TexDev sky; sky.rgba = c->tex[BHRAY_TEX_SKY]; sky.w = c->tex_w[BHRAY_TEX_SKY]; sky.h = c->tex_h[BHRAY_TEX_SKY];
        HIPCHK(c, launch_sky(sky, c->q_dout, (uint2*)c->q_din, n, c->q_stream));
        HIPCHK(c, hipMemcpyAsync(c->q_hin, c->q_din, (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost, c->q_stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->q_stream));
    {   // the kernels' error word, as dev_sync reads it for the frames
        int e = 0;
        HIPCHK(c, hipMemcpy(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost));
        if (e != 0) {
            HIPCHK(c, hipMemset(c->d_err, 0, sizeof(int)));
            return fail(c, e, "kernel reported: %s", bhray_strerror(e));
        }
    }
    if (out) memcpy(out, c->q_hout, (size_t)n * sizeof(float4));
    if (records) memcpy(records, c->q_hrec, (size_t)n * sizeof(bhray_ray_record));
    if (paths) { memcpy(paths->points, c->q_hpts, npts * sizeof(bhray_path_point)); memcpy(paths->counts, c->q_hcnt, (size_t)n * sizeof(uint32_t)); }
    if (sky16) memcpy(sky16, c->q_hin, (size_t)n * sizeof(uint2));
    return BHRAY_OK;
}

// d_records: NULL (bhray_trace_rays_device), or n records, 16-byte aligned (bhray_trace_rays_records_device, whose entry refuses a NULL)
// paths: NULL, or the path outputs in device memory (bhray_trace_rays_paths_device: d_records is then not NULL) - points 16-byte aligned, counts 4-byte aligned
int dev_trace_rays_device(bhray_dev* c, const void* d_rays, uint32_t n, void* d_out, void* d_records, hipStream_t s, const bhray_dev_paths* paths) {
    if (!c) return BHRAY_E_INVALID;
    if (n > BHRAY_MAX_RAYS_PER_CALL || (n != 0 && (!d_rays || !d_out))) return fail(c, BHRAY_E_INVALID, "bhray_trace_rays_device: bad arguments");
    if (((uintptr_t)d_rays | (uintptr_t)d_out | (uintptr_t)d_records) & 15u) return fail(c, BHRAY_E_INVALID, "bhray_trace_rays_device: the arrays must be 16-byte aligned");
    if (paths && (paths->max_points < 2u || paths->stride_log2 > BHRAY_MAX_PATH_STRIDE_LOG2 || (uint64_t)n * paths->max_points > BHRAY_MAX_PATH_POINTS_PER_CALL ||
                  (n != 0 && (!paths->points || !paths->counts || !d_records)) || ((uintptr_t)paths->points & 15u) || ((uintptr_t)paths->counts & 3u)))
        return fail(c, BHRAY_E_INVALID, "bhray_trace_rays_paths_device: bad arguments");
    { int rc = rays_refused(c, "bhray_trace_rays_device", paths != nullptr); if (rc) return rc; }
    if (n == 0) return BHRAY_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = ensure_query(c); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(c->q_begin, s));                     // the batch starts behind what `s` holds now ...
    HIPCHK(c, hipStreamWaitEvent(c->q_stream, c->q_begin, 0));
    PathArgs pa{};
    if (paths) pa = PathArgs{paths->points, paths->counts, paths->stride_log2, paths->max_points};
    { int rc = enqueue_rays(c, (const float4*)d_rays, n, (float4*)d_out, d_records, paths ? &pa : nullptr); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(c->q_done, c->q_stream));            // ... and what `s` gets from now on starts behind the batch
    HIPCHK(c, hipStreamWaitEvent(s, c->q_done, 0));
    return BHRAY_OK;
}

// ---- the accumulation image (include/bhray.h: bhray_accum_*) ----------------------------------------------------
// Sub-pixel samples of every frame pixel, generated, traced (enqueue_rays: the ray-list kernels), resolved and summed on the query stream, so whatever waits for
// the ray batches (sync_all, dev_destroy) waits for the accumulation too.
namespace {
constexpr uint32_t ACCUM_LAUNCH_RAYS = 1u << 22;                  // rays per trace launch unless dev_accum_set_launch_rays says otherwise
int display_whole_frame(bhray_dev* c);                            // (with the frame images, below)

// what a ctx is created with and keeps: refused by every accumulation call
int accum_refused(bhray_dev* c, const char* name) {
    if (c->cfg.flags & (BHRAY_F_LITERAL | BHRAY_F_EVAL_FMA)) return fail(c, BHRAY_E_STATE, "%s: no ray-list kernel for BHRAY_F_LITERAL / BHRAY_F_EVAL_FMA", name);
    if (c->cfg.row_world > 1 || c->local_rows.size() != (size_t)c->cfg.frame_h)
        return fail(c, BHRAY_E_STATE, "%s: the accumulation needs the whole frame: this ctx renders %zu of %u rows", name, c->local_rows.size(), c->cfg.frame_h);
    return BHRAY_OK;
}

// the query stream's work is complete, and the kernels' error word as dev_sync reads it for the frames
int query_wait(bhray_dev* c) {
    HIPCHK(c, hipStreamSynchronize(c->q_stream));
    int e = 0;
    HIPCHK(c, hipMemcpy(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost));
    if (e != 0) {
        HIPCHK(c, hipMemset(c->d_err, 0, sizeof(int)));
        return fail(c, e, "kernel reported: %s", bhray_strerror(e));
    }
    return BHRAY_OK;
}

// the generator's arguments under the current uniforms: the camera members of a frame's FrameParams, the last level's constants with create_ray's operations
void accum_gen_args(bhray_dev* c, AccumGen& g) {
    FrameParams P;
    derive_frame(c, P);
    memset(&g, 0, sizeof g);
    memcpy(g.cam, P.cam, 12); memcpy(g.right, P.right, 12); memcpy(g.up, P.up, 12); memcpy(g.fwd_ff, P.fwd_ff, 12);
    const int lw = (int)c->cfg.level_w[c->cfg.levels - 1], lh = (int)c->cfg.level_h[c->cfg.levels - 1];
    const int sm = (lw - 1) < (lh - 1) ? (lw - 1) : (lh - 1);
    g.half_w = (float)(lw - 1) * 0.5f; g.half_h = (float)(lh - 1) * 0.5f;
    g.increment = 1.0f / (float)sm;
    g.crop_x = c->cfg.crop_x; g.crop_y = c->cfg.crop_y; g.frame_w = c->cfg.frame_w;
    g.npix = c->cfg.frame_w * c->cfg.frame_h;
}

// a_rays / a_res hold `need` rays: grow-only, behind a wait for the stream
int accum_staging(bhray_dev* c, size_t need) {
    if (need <= c->a_cap) return BHRAY_OK;
    HIPCHK(c, hipStreamSynchronize(c->q_stream));
    if (c->a_rays) (void)hipFree(c->a_rays);
    if (c->a_res) (void)hipFree(c->a_res);
    c->a_rays = c->a_res = nullptr; c->a_cap = 0;
    HIPCHK(c, hipMalloc(&c->a_rays, need * sizeof(bhray_ray)));
    HIPCHK(c, hipMalloc(&c->a_res, need * sizeof(float4)));
    c->a_cap = need;
    return BHRAY_OK;
}

// still passes: a_rec holds `need` records and, under a tent or a cubic, a_pimg `need` texels: grow-only, behind a wait for the stream
int accum_pass_staging(bhray_dev* c, size_t need, bool filtered) {
    if (need > c->a_rec_cap) {
        HIPCHK(c, hipStreamSynchronize(c->q_stream));
        if (c->a_rec) (void)hipFree(c->a_rec);
        c->a_rec = nullptr; c->a_rec_cap = 0;
        HIPCHK(c, hipMalloc(&c->a_rec, need * sizeof(bhray_ray_record)));
        c->a_rec_cap = need;
    }
    if (filtered && need > c->a_pimg_cap) {
        HIPCHK(c, hipStreamSynchronize(c->q_stream));
        if (c->a_pimg) (void)hipFree(c->a_pimg);
        c->a_pimg = nullptr; c->a_pimg_cap = 0;
        HIPCHK(c, hipMalloc(&c->a_pimg, need * sizeof(float4)));
        c->a_pimg_cap = need;
    }
    return BHRAY_OK;
}
}  // namespace

int dev_accum_begin(bhray_dev* c) {
    if (!c) return BHRAY_E_INVALID;
    { int rc = accum_refused(c, "bhray_accum_begin"); if (rc) return rc; }
    const size_t npix = (size_t)c->cfg.frame_w * c->cfg.frame_h;
    if (npix > BHRAY_MAX_RAYS_PER_CALL) return fail(c, BHRAY_E_INVALID, "bhray_accum_begin: the frame has more pixels than a ray batch holds");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = ensure_query(c); if (rc) return rc; }
    if (!c->a_sum) HIPCHK(c, hipMalloc(&c->a_sum, npix * sizeof(float4)));
    if (!c->a_mean) HIPCHK(c, hipMalloc(&c->a_mean, npix * sizeof(float4)));
    HIPCHK(c, hipMemsetAsync(c->a_sum, 0, npix * sizeof(float4), c->q_stream));          // behind the samples of the accumulation before
    if (c->a_state) HIPCHK(c, hipMemsetAsync(c->a_state, 0, npix * sizeof(uint4), c->q_stream));
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) {             // still passes: the set is fixed here; one cleared plane per pass
        if (!((c->a_passes_next >> b) & 1u)) continue;
        if (!c->a_pass[b]) HIPCHK(c, hipMalloc(&c->a_pass[b], npix * sizeof(float4)));
        HIPCHK(c, hipMemsetAsync(c->a_pass[b], 0, npix * sizeof(float4), c->q_stream));
    }
    c->a_passes = c->a_passes_next;
    c->a_samples = 0;
    c->a_mode = 0; c->a_min = c->a_round = 0;
    c->a_begun = true;
    return BHRAY_OK;
}

int dev_accum_add(bhray_dev* c, uint32_t samples) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_add: bhray_accum_begin has not been called");
    { int rc = accum_refused(c, "bhray_accum_add"); if (rc) return rc; }
    { int rc = rays_refused(c, "bhray_accum_add"); if (rc) return rc; }
    if (c->a_mode == 2) return fail(c, BHRAY_E_STATE, "bhray_accum_add: this accumulation is adaptive (bhray_accum_add_adaptive); bhray_accum_begin starts another");
    if (samples > BHRAY_ACCUM_MAX_SAMPLES - c->a_samples)
        return fail(c, BHRAY_E_INVALID, "bhray_accum_add: %u + %u samples exceed BHRAY_ACCUM_MAX_SAMPLES", c->a_samples, samples);
    const bool starred = c->a_stars && c->stars.stars;            // point stars in stills: the switch is on and a catalogue is in force
    if (starred && c->a_cam.lens_radius > 0.0f)
        return fail(c, BHRAY_E_STATE, "bhray_accum_add: point stars (bhray_accum_set_stars) under a lens: neighbouring pixels look through different lens points, so their "
                                      "escape directions bound no footprint");
    if (samples == 0) return BHRAY_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }              // the staged frames first: they keep the uniforms they were staged with
    { int rc = ensure_query(c); if (rc) return rc; }
    AccumGen g;
    accum_gen_args(c, g);
    const bool still = !still_camera_is_default(c->a_cam);        // another projection or a lens: bhray_stillcam.hip's generator in accum_gen_kernel's place
    StillGen sg;
    const bool moving = !observer_at_rest(c->a_obs);              // an observer in force: bhray_observer.hip's generator, through still_gen_fill of whichever camera
    ObserverDev ob{};
    if (moving) observer_fill(ob, c->a_obs);
    if (moving || still) still_gen_fill(sg, c->cfg, c->cam, c->a_cam);
    const bool filtered = c->a_filter.kind != BHRAY_FILTER_BOX;   // a tent or a cubic: bhray_accum_filter.hip's stencil in accum_add_kernel's place
    AccumFilter af;
    if (filtered) accum_filter_fill(af, c->a_filter);
    const uint32_t launch_rays = c->a_launch_rays ? c->a_launch_rays : ACCUM_LAUNCH_RAYS;
    const uint32_t kmax = std::max<uint32_t>(1u, launch_rays / g.npix);                   // a small frame takes several samples per launch: the device stays filled
    { int rc = accum_staging(c, (size_t)std::min(samples, kmax) * g.npix); if (rc) return rc; }
    const uint32_t passes = c->a_passes;                          // still passes: 0 - every launch below is the one it was
    if (passes) { int rc = accum_pass_staging(c, (size_t)std::min(samples, kmax) * g.npix, filtered); if (rc) return rc; }
    AccumPassPlanes planes;
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) planes.plane[b] = (passes >> b) & 1u ? c->a_pass[b] : nullptr;
    TexDev sky; sky.rgba = c->tex[BHRAY_TEX_SKY]; sky.w = c->tex_w[BHRAY_TEX_SKY]; sky.h = c->tex_h[BHRAY_TEX_SKY];
    // a whole 360 degree panorama is periodic in x (lon(x + lw) = lon(x) + 2 pi): its first and last columns are neighbours for the stars' footprints
    const int star_wrap = c->a_cam.projection == BHRAY_STILL_EQUIRECT && c->cfg.crop_x == 0 && c->cfg.frame_w == c->cfg.level_w[c->cfg.levels - 1];
    for (uint32_t left = samples; left != 0;) {                   // in stream order: launch i + 1 rewrites the staging behind launch i's add
        const uint32_t k = std::min(left, kmax);
        g.s0 = c->a_samples; g.k = k;
        if (moving) { sg.a.s0 = g.s0; sg.a.k = k; HIPCHK(c, launch_observer_gen(sg, ob, c->a_rays, c->q_stream)); }
        else if (still) { sg.a.s0 = g.s0; sg.a.k = k; HIPCHK(c, launch_still_gen(sg, c->a_rays, c->q_stream)); }
        else HIPCHK(c, launch_accum_gen(g, c->a_rays, c->q_stream));
        { int rc = enqueue_rays(c, c->a_rays, k * g.npix, c->a_res, passes ? (void*)c->a_rec : nullptr); if (rc) return rc; }
        if (passes && !filtered) HIPCHK(c, launch_accum_passes_add(c->a_res, c->a_rec, c->a_rays, planes, passes, g.npix, k, c->q_stream));
        else if (passes) {                                        // before the star stage: it overwrites the ray staging, whose directions the escape pass reads
            for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) {
                if (!((passes >> b) & 1u)) continue;
                HIPCHK(c, launch_accum_passes_form(c->a_res, c->a_rec, c->a_rays, 1u << b, c->a_pimg, (size_t)k * g.npix, c->q_stream));
                HIPCHK(c, launch_accum_filter_add(sky, af, c->a_pimg, c->a_pass[b], c->cfg.frame_w, c->cfg.frame_h, g.s0, k, c->q_stream));
            }
        }
        float4* res = c->a_res;
        if (starred) {                                            // the starred images T go where the launch's records were: dead in stream order until the next generator
            HIPCHK(c, launch_accum_stars(c->stars, sky, c->a_res, c->a_rays, c->cfg.frame_w, c->cfg.frame_h, k, star_wrap, c->q_stream));
            res = c->a_rays;
        }
        if (moving && c->a_obs.beaming == 1u) HIPCHK(c, launch_observer_beam(sg, ob, sky, res, c->q_stream));   // D^4 onto whichever buffer the add reads
        if (filtered) HIPCHK(c, launch_accum_filter_add(sky, af, res, c->a_sum, c->cfg.frame_w, c->cfg.frame_h, g.s0, k, c->q_stream));
        else HIPCHK(c, launch_accum_add(sky, res, c->a_sum, g.npix, k, c->q_stream));
        c->a_samples += k; left -= k;
        c->a_mode = 1;
    }
    return BHRAY_OK;
}

// ---- adaptive stills (include/bhray.h: bhray_accum_add_adaptive) -------------------------------------------------
namespace {
int adaptive_params_bad(bhray_dev* c, const char* name, const bhray_accum_adaptive* a) {
    if (!a) return fail(c, BHRAY_E_INVALID, "%s: NULL params", name);
    if (a->struct_size != sizeof(bhray_accum_adaptive)) return fail(c, BHRAY_E_INVALID, "%s: struct_size %u, expected %zu", name, a->struct_size, sizeof(bhray_accum_adaptive));
    if (a->min_samples < 2 || a->max_samples < a->min_samples || a->max_samples > BHRAY_ACCUM_MAX_SAMPLES || a->round_samples == 0 ||
        (a->max_samples - a->min_samples) % a->round_samples != 0)
        return fail(c, BHRAY_E_INVALID, "%s: min_samples %u, max_samples %u, round_samples %u: need 2 <= min <= max <= %u, round >= 1 and (max - min) %% round == 0", name,
                    a->min_samples, a->max_samples, a->round_samples, BHRAY_ACCUM_MAX_SAMPLES);
    if (!std::isfinite(a->tolerance) || !std::isfinite(a->dark) || a->tolerance < 0.0f || a->dark < 0.0f)
        return fail(c, BHRAY_E_INVALID, "%s: tolerance and dark must be finite and >= 0", name);
    if (c->a_mode == 2 && (a->min_samples != c->a_min || a->round_samples != c->a_round))
        return fail(c, BHRAY_E_INVALID, "%s: min_samples %u / round_samples %u differ from this accumulation's %u / %u", name, a->min_samples, a->round_samples, c->a_min, c->a_round);
    return BHRAY_OK;
}

// the state records, the list and the control block: allocated on first use, the records cleared behind whatever the stream holds
int ensure_adaptive(bhray_dev* c) {
    const size_t npix = (size_t)c->cfg.frame_w * c->cfg.frame_h;
    if (!c->a_state) {
        HIPCHK(c, hipMalloc(&c->a_state, npix * sizeof(uint4)));
        HIPCHK(c, hipMemsetAsync(c->a_state, 0, npix * sizeof(uint4), c->q_stream));
    }
    if (!c->a_list) HIPCHK(c, hipMalloc(&c->a_list, npix * sizeof(uint32_t)));
    if (!c->a_ctl) HIPCHK(c, hipMalloc(&c->a_ctl, 2 * sizeof(uint32_t)));
    if (!c->a_hctl) HIPCHK(c, hipHostMalloc(&c->a_hctl, 2 * sizeof(uint32_t)));
    return BHRAY_OK;
}

// one selection: clear the control block, select, copy the block to the pinned word and wait for it.  n: pixels selected, top: the largest issued among them
int adaptive_select(bhray_dev* c, const bhray_accum_adaptive& a, uint32_t& n, uint32_t& top) {
    const uint32_t npix = c->cfg.frame_w * c->cfg.frame_h;
    HIPCHK(c, hipMemsetAsync(c->a_ctl, 0, 2 * sizeof(uint32_t), c->q_stream));
    HIPCHK(c, launch_adapt_select(c->a_sum, c->a_state, npix, a.max_samples, a.tolerance, a.dark, c->a_list, c->a_ctl, c->q_stream));
    HIPCHK(c, hipMemcpyAsync(c->a_hctl, c->a_ctl, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->q_stream));
    HIPCHK(c, hipStreamSynchronize(c->q_stream));
    n = c->a_hctl[0]; top = c->a_hctl[1];
    if (n > npix) return fail(c, BHRAY_E_HIP, "the adaptive selection returned %u of %u pixels", n, npix);
    return BHRAY_OK;
}

// `count` more samples for the n listed pixels (list == nullptr: every pixel), in chunks of launch_rays / n sub-samples: gen, trace, add; the last add advances issued
// (sg != nullptr: the still camera's list generator in adapt_gen_kernel's place; ob != nullptr, then with sg: the observer's, and its beam stage when `beam`)
int adaptive_round(bhray_dev* c, AccumGen& g, StillGen* sg, const ObserverDev* ob, bool beam, const TexDev& sky, const uint32_t* list, uint32_t n, uint32_t count) {
    const uint32_t launch_rays = c->a_launch_rays ? c->a_launch_rays : ACCUM_LAUNCH_RAYS;
    const uint32_t kmax = std::max<uint32_t>(1u, launch_rays / n);
    { int rc = accum_staging(c, (size_t)std::min(count, kmax) * n); if (rc) return rc; }
    for (uint32_t j0 = 0; j0 < count;) {                          // in stream order: chunk i + 1 rewrites the staging behind chunk i's add
        const uint32_t k = std::min(count - j0, kmax);
        g.k = k;
        if (ob) { sg->a.k = k; HIPCHK(c, launch_observer_gen_list(*sg, *ob, list, n, j0, c->a_state, c->a_rays, c->q_stream)); }
        else if (sg) { sg->a.k = k; HIPCHK(c, launch_still_gen_list(*sg, list, n, j0, c->a_state, c->a_rays, c->q_stream)); }
        else HIPCHK(c, launch_adapt_gen(g, list, n, j0, c->a_state, c->a_rays, c->q_stream));
        { int rc = enqueue_rays(c, c->a_rays, k * n, c->a_res); if (rc) return rc; }
        if (ob && beam) HIPCHK(c, launch_observer_beam_list(*sg, *ob, sky, list, n, j0, c->a_state, c->a_res, c->q_stream));   // before j0 moves: the generator's indices
        j0 += k;
        HIPCHK(c, launch_adapt_add(sky, c->a_res, list, n, k, j0 == count ? count : 0u, c->a_sum, c->a_state, c->q_stream));
    }
    return BHRAY_OK;
}
}  // namespace

int dev_accum_add_adaptive(bhray_dev* c, const bhray_accum_adaptive* params, bhray_accum_adaptive_info* info) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_add_adaptive: bhray_accum_begin has not been called");
    { int rc = accum_refused(c, "bhray_accum_add_adaptive"); if (rc) return rc; }
    { int rc = rays_refused(c, "bhray_accum_add_adaptive"); if (rc) return rc; }
    if (c->a_mode == 1) return fail(c, BHRAY_E_STATE, "bhray_accum_add_adaptive: this accumulation holds bhray_accum_add's samples; bhray_accum_begin starts another");
    if (c->a_passes) return fail(c, BHRAY_E_STATE, "bhray_accum_add_adaptive: this accumulation carries still passes (bhray_accum_set_passes): the adaptive adder works over a "
                                                   "pixel list, and no list form of the passes is built");
    if (c->a_filter.kind != BHRAY_FILTER_BOX)
        return fail(c, BHRAY_E_STATE, "bhray_accum_add_adaptive: a still filter other than the box is in force (bhray_accum_set_filter): a round's pixels take different samples");
    if (c->a_stars && c->stars.stars)
        return fail(c, BHRAY_E_STATE, "bhray_accum_add_adaptive: point stars are on (bhray_accum_set_stars) and a catalogue is in force: a round's pixels take different samples, "
                                      "so a neighbour has no direction for \"sample s\"");
    { int rc = adaptive_params_bad(c, "bhray_accum_add_adaptive", params); if (rc) return rc; }
    const bhray_accum_adaptive a = *params;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }              // the staged frames first: they keep the uniforms they were staged with
    { int rc = ensure_query(c); if (rc) return rc; }
    { int rc = ensure_adaptive(c); if (rc) return rc; }
    AccumGen g;
    accum_gen_args(c, g);
    StillGen sgen;
    StillGen* sg = nullptr;
    const bool moving = !observer_at_rest(c->a_obs);              // an observer in force: its generators, through still_gen_fill of whichever camera
    if (moving || !still_camera_is_default(c->a_cam)) { still_gen_fill(sgen, c->cfg, c->cam, c->a_cam); sg = &sgen; }
    ObserverDev obd{};
    const ObserverDev* ob = nullptr;
    if (moving) { observer_fill(obd, c->a_obs); ob = &obd; }
    const bool beam = moving && c->a_obs.beaming == 1u;
    TexDev sky; sky.rgba = c->tex[BHRAY_TEX_SKY]; sky.w = c->tex_w[BHRAY_TEX_SKY]; sky.h = c->tex_h[BHRAY_TEX_SKY];
    bhray_accum_adaptive_info I{};
    if (c->a_mode == 0) {                                         // the first round: every pixel, no test
        { int rc = adaptive_round(c, g, sg, ob, beam, sky, nullptr, g.npix, a.min_samples); if (rc) return rc; }
        c->a_mode = 2; c->a_min = a.min_samples; c->a_round = a.round_samples; c->a_samples = a.min_samples;
        I.rounds = 1; I.rays = (uint64_t)g.npix * a.min_samples;
    }
    for (;;) {
        uint32_t n = 0, top = 0;
        { int rc = adaptive_select(c, a, n, top); if (rc) return rc; }
        I.active_last = n;
        if (n == 0) break;
        { int rc = adaptive_round(c, g, sg, ob, beam, sky, c->a_list, n, a.round_samples); if (rc) return rc; }
        c->a_samples = std::max(c->a_samples, top + a.round_samples);
        I.rounds++; I.rays += (uint64_t)n * a.round_samples;
    }
    I.reach = c->a_samples;
    if (info) *info = I;
    return BHRAY_OK;
}

int dev_accum_read_counts(bhray_dev* c, uint32_t* dst, size_t pitch) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_read_counts: bhray_accum_begin has not been called");
    if (c->a_mode != 2) return fail(c, BHRAY_E_STATE, "bhray_accum_read_counts: this accumulation is not adaptive");
    const size_t rowb = (size_t)c->cfg.frame_w * sizeof(uint32_t);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_adapt_counts(c->a_state, c->a_list, c->cfg.frame_w * c->cfg.frame_h, c->q_stream));   // (the list is idle between two selections)
    { int rc = query_wait(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpy2D(dst, pitch, c->a_list, rowb, rowb, c->cfg.frame_h, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// bhray_diag.h: one selection under `params`, no sampling
int dev_accum_active_pixels(bhray_dev* c, const bhray_accum_adaptive* params, uint32_t* out, uint32_t cap, uint32_t* n_out) {
    if (!c) return BHRAY_E_INVALID;
    if (!n_out || (cap != 0 && !out)) return fail(c, BHRAY_E_INVALID, "bhray_accum_active_pixels: bad arguments");
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_active_pixels: bhray_accum_begin has not been called");
    { int rc = accum_refused(c, "bhray_accum_active_pixels"); if (rc) return rc; }
    if (c->a_mode == 1) return fail(c, BHRAY_E_STATE, "bhray_accum_active_pixels: this accumulation is not adaptive");
    { int rc = adaptive_params_bad(c, "bhray_accum_active_pixels", params); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = ensure_query(c); if (rc) return rc; }
    { int rc = ensure_adaptive(c); if (rc) return rc; }
    uint32_t n = 0, top = 0;
    { int rc = adaptive_select(c, *params, n, top); if (rc) return rc; }
    *n_out = n;
    const uint32_t m = std::min(n, cap);
    if (m) HIPCHK(c, hipMemcpy(out, c->a_list, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

int dev_accum_samples(const bhray_dev* c, uint32_t* total) {
    if (!c || !total) return BHRAY_E_INVALID;
    *total = c->a_samples;
    return BHRAY_OK;
}

int dev_accum_read(bhray_dev* c, float* dst, size_t pitch) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_read: bhray_accum_begin has not been called");
    const size_t rowb = (size_t)c->cfg.frame_w * sizeof(float4);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_accum_mean(c->a_sum, c->a_mean, nullptr, c->cfg.frame_w * c->cfg.frame_h, c->q_stream));
    { int rc = query_wait(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpy2D(dst, pitch, c->a_mean, rowb, rowb, c->cfg.frame_h, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// still passes: validates and stores - no device call; the next dev_accum_begin takes the set
int dev_accum_set_passes(bhray_dev* c, uint32_t passes) {
    if (!c) return BHRAY_E_INVALID;
    if (passes & ~(uint32_t)BHRAY_PASS_ALL) return fail(c, BHRAY_E_INVALID, "bhray_accum_set_passes: unknown pass bits 0x%x", passes & ~(uint32_t)BHRAY_PASS_ALL);
    c->a_passes_next = passes;
    return BHRAY_OK;
}

int dev_accum_passes(const bhray_dev* c, uint32_t* passes) {
    if (!c || !passes) return BHRAY_E_INVALID;
    *passes = c->a_begun ? c->a_passes : 0u;
    return BHRAY_OK;
}

// the mean of one pass's plane: dev_accum_read's kernel and copy over that plane
int dev_accum_read_pass(bhray_dev* c, uint32_t pass, float* dst, size_t pitch) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_read_pass: bhray_accum_begin has not been called");
    if (pass == 0 || (pass & (pass - 1)) != 0 || (pass & c->a_passes) != pass)
        return fail(c, BHRAY_E_INVALID, "bhray_accum_read_pass: pass 0x%x is not one pass of this accumulation's set 0x%x", pass, c->a_passes);
    const size_t rowb = (size_t)c->cfg.frame_w * sizeof(float4);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    uint32_t b = 0;
    while (!((pass >> b) & 1u)) b++;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_accum_mean(c->a_pass[b], c->a_mean, nullptr, c->cfg.frame_w * c->cfg.frame_h, c->q_stream));
    { int rc = query_wait(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpy2D(dst, pitch, c->a_mean, rowb, rowb, c->cfg.frame_h, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// mean -> RGBA16F -> the display pass (launch_display, unchanged) with the ctx's post uniforms -> RGBA8
int dev_accum_read_display(bhray_dev* c, uint8_t* dst, size_t pitch, const bhray_fxaa_details* fx, const bhray_mix_details* mx) {
    if (!c || !fx || !mx) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_read_display: bhray_accum_begin has not been called");
    { int rc = display_whole_frame(c); if (rc) return rc; }
    const size_t rowb = (size_t)c->cfg.frame_w * sizeof(uint32_t);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t npix = c->cfg.frame_w * c->cfg.frame_h;
    if (!c->a_mean16) HIPCHK(c, hipMalloc(&c->a_mean16, (size_t)npix * sizeof(uint2)));
    if (!c->a_scratch) HIPCHK(c, hipMalloc(&c->a_scratch, display_scratch_bytes(c->cfg.frame_w, c->cfg.frame_h)));
    if (!c->a_disp) HIPCHK(c, hipMalloc(&c->a_disp, (size_t)npix * sizeof(uint32_t)));
    HIPCHK(c, launch_accum_mean(c->a_sum, c->a_mean, c->a_mean16, npix, c->q_stream));
    HIPCHK(c, launch_display(c->a_mean16, c->a_scratch, c->a_disp, c->cfg.frame_w, c->cfg.frame_h, *fx, *mx, c->q_stream));
    { int rc = query_wait(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpy2D(dst, pitch, c->a_disp, rowb, rowb, c->cfg.frame_h, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// Denoised stills: prepare, then one a-trous launch per iteration, on the query stream behind the samples.  Reads a_sum and the pass planes, writes
// a_mean and the filter's own images: no accumulation state changes.  The answer is left in *result; with `display`, its RGBA16F rounding in a_mean16.
namespace {
// ev (may be nullptr): 2 + iterations events, recorded before the prepare launch and behind every launch (dev_accum_denoise_times).
int accum_denoise_enqueue(bhray_dev* c, const char* name, const bhray_still_denoise* p, bool display, float4** result, hipEvent_t* ev = nullptr) {
    if (c->a_passes == 0) return fail(c, BHRAY_E_STATE, "%s: this accumulation carries no still passes (bhray_accum_set_passes before bhray_accum_begin): the filter has no guide", name);
    if (c->a_mode == 2) return fail(c, BHRAY_E_STATE, "%s: this accumulation is adaptive", name);
    bhray_still_denoise defaults;
    if (!p) { bhray_still_denoise_default(&defaults); p = &defaults; }
    if (const char* why = still_denoise_error(p, c->a_passes)) return fail(c, BHRAY_E_INVALID, "%s: %s (the set is 0x%x)", name, why, c->a_passes);
    DenoiseRule rule;
    denoise_rule_fill(rule, p, c->a_passes);
    const uint32_t npix = c->cfg.frame_w * c->cfg.frame_h;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 2; i++) if (!c->a_dn[i]) HIPCHK(c, hipMalloc(&c->a_dn[i], (size_t)npix * sizeof(float4)));
    const uint32_t needs[3] = {DENOISE_NEEDS_G0, DENOISE_NEEDS_G1, DENOISE_NEEDS_G2};
    for (int i = 0; i < 3; i++) if ((rule.guides & needs[i]) && !c->a_dng[i]) HIPCHK(c, hipMalloc(&c->a_dng[i], (size_t)npix * sizeof(float4)));
    if (display && !c->a_mean16) HIPCHK(c, hipMalloc(&c->a_mean16, (size_t)npix * sizeof(uint2)));
    AccumPassPlanes planes;
    for (uint32_t b = 0; b < ACCUM_PASS_COUNT; b++) planes.plane[b] = (rule.guides >> b) & 1u ? c->a_pass[b] : nullptr;
    float4* g[3];
    for (int i = 0; i < 3; i++) g[i] = (rule.guides & needs[i]) ? c->a_dng[i] : nullptr;
    if (ev) HIPCHK(c, hipEventRecord(ev[0], c->q_stream));
    HIPCHK(c, launch_denoise_prepare(c->a_sum, planes, rule.guides, c->a_mean, c->a_dn[0], g[0], g[1], g[2], npix, c->q_stream));
    if (ev) HIPCHK(c, hipEventRecord(ev[1], c->q_stream));
    for (uint32_t it = 0; it < p->iterations; it++) {
        const bool last = it + 1 == p->iterations;
        HIPCHK(c, launch_denoise_atrous(rule, c->a_dn[it & 1], g[0], g[1], g[2], c->a_mean, c->a_dn[(it + 1) & 1], last && display ? c->a_mean16 : nullptr,
                                        c->cfg.frame_w, c->cfg.frame_h, 1u << it, last, c->q_stream));
        if (ev) HIPCHK(c, hipEventRecord(ev[2 + it], c->q_stream));
    }
    *result = c->a_dn[p->iterations & 1];
    return BHRAY_OK;
}
}  // namespace

int dev_accum_read_denoised(bhray_dev* c, const bhray_still_denoise* p, float* dst, size_t pitch) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_read_denoised: bhray_accum_begin has not been called");
    const size_t rowb = (size_t)c->cfg.frame_w * sizeof(float4);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    float4* result = nullptr;
    { int rc = accum_denoise_enqueue(c, "bhray_accum_read_denoised", p, false, &result); if (rc) return rc; }
    { int rc = query_wait(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpy2D(dst, pitch, result, rowb, rowb, c->cfg.frame_h, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// bhray_diag.h: the launches of dev_accum_read_denoised with an event between them; delivers no image
int dev_accum_denoise_times(bhray_dev* c, const bhray_still_denoise* p, float ms[6]) {
    if (!c) return BHRAY_E_INVALID;
    if (!ms) return fail(c, BHRAY_E_INVALID, "bhray_accum_denoise_times: NULL ms");
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_denoise_times: bhray_accum_begin has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    hipEvent_t ev[2 + BHRAY_DENOISE_MAX_ITERATIONS] = {};
    int rc = BHRAY_OK;
    for (hipEvent_t& e : ev) if (hipEventCreate(&e) != hipSuccess) rc = fail(c, BHRAY_E_HIP, "bhray_accum_denoise_times: hipEventCreate failed");
    float4* result = nullptr;
    if (!rc) rc = accum_denoise_enqueue(c, "bhray_accum_denoise_times", p, false, &result, ev);
    if (!rc) rc = query_wait(c);
    if (!rc) {
        const uint32_t iterations = p ? p->iterations : 0;        // nullptr: the defaults'
        bhray_still_denoise d;
        bhray_still_denoise_default(&d);
        const uint32_t n = iterations ? iterations : d.iterations;
        for (uint32_t i = 0; i < 1 + BHRAY_DENOISE_MAX_ITERATIONS; i++) {
            ms[i] = 0.0f;
            if (i < 1 + n && hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = fail(c, BHRAY_E_HIP, "bhray_accum_denoise_times: hipEventElapsedTime failed");
        }
    }
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    return rc;
}

// denoised mean -> RGBA16F (the last a-trous launch) -> the display pass (launch_display, unchanged) with the ctx's post uniforms -> RGBA8
int dev_accum_read_display_denoised(bhray_dev* c, const bhray_still_denoise* p, uint8_t* dst, size_t pitch, const bhray_fxaa_details* fx, const bhray_mix_details* mx) {
    if (!c || !fx || !mx) return BHRAY_E_INVALID;
    if (!c->a_begun) return fail(c, BHRAY_E_STATE, "bhray_accum_read_display_denoised: bhray_accum_begin has not been called");
    { int rc = display_whole_frame(c); if (rc) return rc; }
    const size_t rowb = (size_t)c->cfg.frame_w * sizeof(uint32_t);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    float4* result = nullptr;
    { int rc = accum_denoise_enqueue(c, "bhray_accum_read_display_denoised", p, true, &result); if (rc) return rc; }
    const uint32_t npix = c->cfg.frame_w * c->cfg.frame_h;
    if (!c->a_scratch) HIPCHK(c, hipMalloc(&c->a_scratch, display_scratch_bytes(c->cfg.frame_w, c->cfg.frame_h)));
    if (!c->a_disp) HIPCHK(c, hipMalloc(&c->a_disp, (size_t)npix * sizeof(uint32_t)));
    HIPCHK(c, launch_display(c->a_mean16, c->a_scratch, c->a_disp, c->cfg.frame_w, c->cfg.frame_h, *fx, *mx, c->q_stream));
    { int rc = query_wait(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpy2D(dst, pitch, c->a_disp, rowb, rowb, c->cfg.frame_h, hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// bhray_diag.h: the generated records of sample s under the current uniforms, frame_w * frame_h of them
int dev_accum_sample_rays(bhray_dev* c, uint32_t s, bhray_ray* out) {
    if (!c) return BHRAY_E_INVALID;
    if (!out || s >= BHRAY_ACCUM_MAX_SAMPLES) return fail(c, BHRAY_E_INVALID, "bhray_accum_sample_rays: bad arguments");
    { int rc = accum_refused(c, "bhray_accum_sample_rays"); if (rc) return rc; }
    if (!c->have_uniforms) return fail(c, BHRAY_E_STATE, "bhray_accum_sample_rays: bhray_set_uniforms has not been called");
    AccumGen g;
    accum_gen_args(c, g);
    if (g.npix > BHRAY_MAX_RAYS_PER_CALL) return fail(c, BHRAY_E_INVALID, "bhray_accum_sample_rays: the frame has more pixels than a ray batch holds");
    g.s0 = s; g.k = 1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = ensure_query(c); if (rc) return rc; }
    float4* d = nullptr;
    HIPCHK(c, hipMalloc(&d, (size_t)g.npix * sizeof(bhray_ray)));
    hipError_t e;
    if (!observer_at_rest(c->a_obs)) {                            // the observer's generator
        StillGen sg;
        still_gen_fill(sg, c->cfg, c->cam, c->a_cam);
        sg.a.s0 = s; sg.a.k = 1;
        ObserverDev ob;
        observer_fill(ob, c->a_obs);
        e = launch_observer_gen(sg, ob, d, c->q_stream);
    }
    else if (still_camera_is_default(c->a_cam)) e = launch_accum_gen(g, d, c->q_stream);
    else {
        StillGen sg;
        still_gen_fill(sg, c->cfg, c->cam, c->a_cam);
        sg.a.s0 = s; sg.a.k = 1;
        e = launch_still_gen(sg, d, c->q_stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->q_stream);
    if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)g.npix * sizeof(bhray_ray), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(c, e);
    return BHRAY_OK;
}

// validates and stores: no device call, no image touched (NULL: the default)
int dev_accum_set_camera(bhray_dev* c, const bhray_still_camera* cam) {
    if (!c) return BHRAY_E_INVALID;
    if (const char* why = still_camera_error(cam)) return fail(c, BHRAY_E_INVALID, "bhray_accum_set_camera: %s", why);
    if (cam) c->a_cam = *cam; else bhray_still_camera_default(&c->a_cam);
    return BHRAY_OK;
}

// validates and stores: no device call, no image touched (NULL: at rest)
int dev_accum_set_observer(bhray_dev* c, const bhray_observer* obs) {
    if (!c) return BHRAY_E_INVALID;
    if (const char* why = observer_error(obs)) return fail(c, BHRAY_E_INVALID, "bhray_accum_set_observer: %s", why);
    if (obs) c->a_obs = *obs; else bhray_observer_default(&c->a_obs);
    return BHRAY_OK;
}

// validates and stores: no device call, no image touched (NULL: the default, the box)
int dev_accum_set_filter(bhray_dev* c, const bhray_still_filter* filter) {
    if (!c) return BHRAY_E_INVALID;
    if (const char* why = still_filter_error(filter)) return fail(c, BHRAY_E_INVALID, "bhray_accum_set_filter: %s", why);
    if (filter) c->a_filter = *filter; else bhray_still_filter_default(&c->a_filter);
    return BHRAY_OK;
}

// validates and stores: no device call, no image touched
int dev_accum_set_stars(bhray_dev* c, int32_t on) {
    if (!c) return BHRAY_E_INVALID;
    if (on != 0 && on != 1) return fail(c, BHRAY_E_INVALID, "bhray_accum_set_stars: on must be 0 or 1");
    c->a_stars = on == 1;
    return BHRAY_OK;
}

int dev_accum_set_launch_rays(bhray_dev* c, uint32_t max_rays) {
    if (!c) return BHRAY_E_INVALID;
    if (max_rays > BHRAY_MAX_RAYS_PER_CALL) return fail(c, BHRAY_E_INVALID, "bhray_accum_set_launch_rays: more rays than a ray batch holds");
    c->a_launch_rays = max_rays;
    return BHRAY_OK;
}

// Another row partition for this engine (bhray_set_partition): same frame, same ladder, other rows.  Everything enqueued so far is
// waited for; the row tables are rewritten in place, the per-frame queues and output buffers grow if the new rows need more.  The level
// images, textures, models and uniforms stay.  The temporal mode's per-pixel history stays too (rows that are new to this partition
// have none: their first frame is the plain ladder's).
int dev_set_partition(bhray_dev* c, uint32_t partition, uint32_t stripe_rows, const uint32_t* slab_row0, uint32_t row_rank, uint32_t row_world) {
    if (!c) return BHRAY_E_INVALID;
    bhray_config n = c->cfg;
    n.partition = partition; n.row_rank = row_rank; n.row_world = row_world;
    if (stripe_rows) n.stripe_rows = stripe_rows;
    if (partition == BHRAY_PARTITION_SLABS) {
        if (!slab_row0 || row_world > BHRAY_MAX_DEVICES) return fail(c, BHRAY_E_INVALID, "bad row partition");
        for (uint32_t p = 0; p <= row_world; p++) n.slab_row0[p] = slab_row0[p];
    }
    if (row_world < 1 || row_rank >= row_world) return fail(c, BHRAY_E_INVALID, "bad row partition");
    if (const char* why = partition_error(n, row_world)) return fail(c, BHRAY_E_INVALID, "bad row partition: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    HIPCHK(c, sync_all(c));
    c->cfg = n;
    for (Slot& S : c->slots) S.launched_frames = 0;           // the work the slots' frames counted belongs to the rows this engine had then (dev_get_work)
    for (Slot& S : c->slots) for (size_t i = 0; i < (size_t)c->batch * BHRAY_LEVEL_GRID_LAUNCHES; i++) S.h_qlen[i] = QLEN_NONE;   // ... and so do the queue lengths their launches reported
    { int rc = build_row_tables(c); if (rc) return rc; }
    return ensure_frame_buffers(c, true);
}

// ------------------------------------------------------------------------------------------
// One batch = the frames staged in a slot.  BatchPlan lays out the argument block (FrameParams[B], then one FrameLaunch[nb] array per
// launch, in the slot's pinned staging) and the launch sequence, one method per ladder mode; launch_batch enqueues it.
// ------------------------------------------------------------------------------------------
namespace {
enum class LaunchKind { classify, trace, predict };
enum class TraceBuild { ctx, latency, dense };            // the build a trace launch asks for: the ctx's trace build (choose_build), or one named
TraceBuild trace_build_of(int v) { return v < 0 ? TraceBuild::ctx : (v ? TraceBuild::dense : TraceBuild::latency); }   // (BHRAY_COARSE_BUILD's -1 / 0 / 1)
// a ladder trace launch's id in bhray_level_grid_info (bhray_diag.h; size_grids sizes its grid by queue length)
constexpr int GRID_ID_NONE = -1, GRID_ID_MERGED = 0, GRID_ID_SUPERSET = BHRAY_MAX_LEVELS + 1;   // MERGED: the speculative levels' launch (and the temporal mode's predicted one)
constexpr int grid_id_level(uint32_t l) { return 1 + (int)l; }
static_assert(GRID_ID_SUPERSET + 1 == BHRAY_LEVEL_GRID_LAUNCHES, "launch ids of bhray_level_grid_info");

struct LaunchArgs { FrameLaunch* h; const FrameLaunch* d; };     // the nb argument entries of a launch: in the pinned staging, and their device address
struct Launch {
    LaunchKind kind; LaunchArgs args; int blocks;
    bool count = false;                // classify, trace: the counting kernels
    bool fixup = false;                // classify: CLASSIFY_FIXUP's kernels
    int levels = 1;                    // predict: levels (blockIdx.z)
    int grid_id = GRID_ID_NONE;        // trace
    TraceVariant variant{};            // trace: the build that runs (resolved)
    int ev_before[2] = {-1, -1}, ev_after[2] = {-1, -1};       // timing events recorded around it (ev_*; -1: none)
    Launch& before(int e) { ev_before[0] = e; return *this; }
    Launch& after(int e0, int e1 = -1) { ev_after[0] = e0; ev_after[1] = e1; return *this; }
};

struct BatchPlan {
    bhray_dev* c;
    Slot& S;
    const uint32_t nb, nl;             // frames staged, ladder levels
    const TraceVariant ctx;            // the ctx's trace build for this batch, as asked for (choose_build)
    const int grid;                    // persistent trace blocks of the ctx's trace build
    const bool timing;                 // this batch carries timing events, in entry `ring` of the ring
    const size_t ring;
    hipStream_t st;
    size_t args_used;
    const bool count = ctx.count;      // BHRAY_F_COUNTERS
    bool overflow = false;             // a launch found no room in the argument block (no entry was written)
    uint32_t own_trace = 0;            // bit l: level l has a trace launch of its own (dev_get_timing)
    std::vector<Launch> seq;
    uint32_t first_normal = 0;         // first level that still needs its own classify + trace pair

    // argument block of the next launch: nb FrameLaunch entries on the host, and their device address
    LaunchArgs next_launch() {
        const size_t bytes = (size_t)nb * sizeof(FrameLaunch);
        if (overflow || args_used + bytes > S.args_cap) { overflow = true; return {nullptr, nullptr}; }
        LaunchArgs a{(FrameLaunch*)(S.h_args + args_used), (const FrameLaunch*)(S.d_args + args_used)};
        args_used += bytes;
        memset(a.h, 0, bytes);
        return a;
    }
    void level_params(const FrameRes& R, uint32_t l, LevelParams& L) const {
        const Level& Lv = c->levels[l];
        const bool last = (l == nl - 1);
        memset(&L, 0, sizeof L);
        L.w = Lv.w; L.h = Lv.h;
        if (l == 0) { L.pw = 1; L.ph = 1; L.rx = 1.0f; L.ry = 1.0f; L.prev = nullptr; }
        else {
            const Level& Pv = c->levels[l - 1];
            L.pw = Pv.w; L.ph = Pv.h; L.prev = R.level_out[l - 1];
            const int sfx = (L.w - 1) / (L.pw - 1), sfy = (L.h - 1) / (L.ph - 1);          // ray.wgsl:185
            L.rx = (float)L.pw / (float)(L.w + (sfx - 1)); L.ry = (float)L.ph / (float)(L.h + (sfy - 1));   // ray.wgsl:187
        }
        if (last) {
            L.out = R.out; L.out_pitch = (int)c->cfg.frame_w; L.out_x0 = (int)c->cfg.crop_x; L.rowmap = Lv.d_rowmap;
            L.x0 = (int)c->cfg.crop_x; L.x1 = (int)(c->cfg.crop_x + c->cfg.frame_w);
        } else {
            L.out = R.level_out[l]; L.out_pitch = Lv.w; L.out_x0 = 0; L.rowmap = nullptr; L.x0 = 0; L.x1 = Lv.w;
        }
        L.rows = (Lv.d_rows_near && R.row_variant >= 0) ? Lv.d_rows_near + (size_t)R.row_variant * Lv.rows.size() : Lv.d_rows;
        L.nrows = (int)Lv.rows.size();
    }
    int classify_blocks(uint32_t l) const {
        const Level& Lv = c->levels[l];
        const int span = (l == nl - 1) ? (int)c->cfg.frame_w : Lv.w;
        const int tiles_x = (span + 7) / 8, tiles_y = ((int)Lv.rows.size() + 7) / 8;
        return ((tiles_x + BHRAY_CLASSIFY_BX - 1) / BHRAY_CLASSIFY_BX) * ((tiles_y + BHRAY_CLASSIFY_BY - 1) / BHRAY_CLASSIFY_BY);
    }
    // counting builds: where the iterations of level l's rows are summed (FrameLaunch::row_work, SpecLevel::row_work)
    unsigned long long* row_work(const FrameRes& R, uint32_t l) const { return (count && R.d_row_work) ? R.d_row_work + c->row_work_off[l] : nullptr; }
    // level l as one of the levels of a merged trace launch: geometry and destination as its own launch would have them
    SpecLevel spec_level(const FrameRes& R, uint32_t l, uint32_t* stamp = nullptr) const {
        LevelParams Lp; level_params(R, l, Lp);
        SpecLevel sl{};
        sl.w = Lp.w; sl.h = Lp.h; sl.out = Lp.out; sl.out_pitch = Lp.out_pitch; sl.out_x0 = Lp.out_x0; sl.rowmap = Lp.rowmap; sl.stamp = stamp;
        sl.row_work = row_work(R, l);
        return sl;
    }
    // the next launch's argument entries: for each staged frame k, entry k holds level l's parameters and what fill(entry, frame) adds
    template <class Fill>
    LaunchArgs args_for(uint32_t l, Fill&& fill) {
        const LaunchArgs a = next_launch();
        if (a.h) for (uint32_t k = 0; k < nb; k++) { level_params(S.fr[k], l, a.h[k].L); fill(a.h[k], S.fr[k]); }
        return a;
    }
    // what a trace launch that asks for `b` asks for
    TraceVariant asked(TraceBuild b) const { TraceVariant v = ctx; if (b != TraceBuild::ctx) v.dense = (b == TraceBuild::dense); return v; }
    int full_device_grid(TraceBuild b) const { return c->num_cus * trace_blocks_per_cu(asked(b)); }
    Launch& classify(LaunchArgs a, uint32_t l, bool counted, bool fixup = false) {
        seq.push_back({LaunchKind::classify, a, classify_blocks(l), counted, fixup});
        return seq.back();
    }
    // level: the level whose trace interval ends behind the launch; -1: the temporal mode's predicted launch
    Launch& trace(LaunchArgs a, int blocks, int grid_id, int level, TraceBuild b = TraceBuild::ctx) {
        seq.push_back({LaunchKind::trace, a, blocks, count});
        Launch& Ln = seq.back();
        Ln.grid_id = grid_id; Ln.variant = trace_resolve(asked(b));
        if (level >= 0) own_trace |= 1u << level;
        return Ln.after(level >= 0 ? ev_level_traced((uint32_t)level) : ev_predicted_end(nl));
    }

    // speculative_levels = ns: every needed pixel of levels 0..ns-1 traced in ONE launch, then classified
    void speculative(uint32_t ns) {
        // (1) every needed pixel of levels 0..ns-1 into ONE level-tagged queue, (2) one trace launch over it,
        // (3) classify levels 1..ns-1 against the traced images.  Queue control words of level 0 serve the merged queue.
        for (uint32_t l = 0; l < ns; l++) {
            Launch& Ln = classify(args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.L.pw = 1; F.L.ph = 1; F.L.prev = nullptr; F.L.tag = (int)l;    // "base case": every pixel is traced
                F.queue = R.spec_queue; F.qctl = R.d_qctl; F.counters = nullptr;
            }), l, false);
            if (l == 0) Ln.before(ev_level_begin(0));
            if (l == ns - 1) Ln.after(ev_level_classified(0));
        }
        trace(args_for(0, [&](FrameLaunch& F, const FrameRes& R) {
            F.SL.n = (int)ns;
            for (uint32_t l = 0; l < ns; l++) { F.SL.l[l] = spec_level(R, l); if (l > 0) F.SL.l[l].out = R.spec_out[l]; }
            F.queue = R.spec_queue; F.qctl = R.d_qctl; F.counters = count ? R.d_counters : nullptr;
        }), grid, GRID_ID_MERGED, 0, ns < nl ? trace_build_of(c->coarse_build) : TraceBuild::ctx);   // (ns < nl always: dev_create)
        for (uint32_t l = 1; l < ns; l++)
            classify(args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.L.spec = R.spec_out[l];
                F.queue = nullptr; F.qctl = R.d_qctl + 2 * l; F.counters = count ? R.d_counters + l : nullptr;
            }), l, count).before(ev_level_begin(l)).after(ev_level_classified(l), ev_level_traced(l));   // no trace launch of its own
        first_normal = ns;
    }

    // BHRAY_F_TEMPORAL: the previous frame's traced set in ONE launch, then the ladder fixes up what that prediction missed
    int temporal() {
        const bool shared_device = c->slots.size() > 1;     // other frames' launches share the device with this batch's
        // Temporal speculation: ONE launch traces, for every level, the pixels the previous frame held in this slot position had
        // to trace (its exact classification recorded them); then the ladder runs as usual, except that a pixel that needs tracing
        // and was delivered by the predicted launch (stamp) is not traced again.  With a perfect prediction the per-level trace
        // launches find empty queues and the chain of dependent long rays collapses into one launch; with no prediction (first
        // frame, scene cut) this is the plain ladder.  Pixels are identical in every case.
        for (uint32_t k = 0; k < nb; k++) {
            FrameRes& R = S.fr[k];
            R.stamp_value++;
            if (R.stamp_value == 0) {                          // 32-bit stamps wrapped: start over with clean images
                for (uint32_t l = 0; l < nl; l++) HIPCHK(c, hipMemsetAsync(R.stamp[l], 0, (size_t)c->levels[l].w * (size_t)c->levels[l].h * sizeof(uint32_t), st));
                R.stamp_value = 1;
            }
        }
        // (0) the prediction: per level, the previous frame's traced set dilated by temporal_radius pixels -> one level-tagged queue
        LaunchArgs pred_first{nullptr, nullptr}; int pred_blocks = 0;
        for (uint32_t l = 0; l < nl; l++) {
            const LaunchArgs a = args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.L.tag = (int)l;
                F.queue = R.pred_queue; F.qctl = R.pred_ctl; F.need = R.need[l]; F.radius = (int)(l + 1 == nl ? c->temporal_radius : c->temporal_radius_coarse);
                F.blocks = classify_blocks(l);
            });
            if (l == 0) pred_first = a;
            pred_blocks = std::max(pred_blocks, classify_blocks(l));
        }
        seq.push_back({LaunchKind::predict, pred_first, pred_blocks});      // ONE launch, blockIdx.z = level (the entries are contiguous)
        seq.back().levels = (int)nl;
        seq.back().before(ev_predicted_begin(nl));
        // the predicted launch holds a whole frame's rays: the dense build (0.61 against 0.66 ms at 1080p); the fix-up launches are
        // expected to be nearly empty: the latency build, which looks at the queue head before its first atomic.
        // Grids: with ONE frame slot the device is this frame's - full-occupancy grids; with several slots the ctx's rule for every
        // trace launch (2 persistent blocks per CU: `grid`) - a full-device persistent grid keeps the next batch's small kernels
        // (its prediction, its fix-up classification) waiting until it has drained, and two batches then run one after the other
        // (rank 3 of an 8-way 1080p partition, 20-frame blocks of a moving sequence: 0.0995 -> 0.0736 ms per frame, EXPERIMENTS R4.12)
        trace(args_for(0, [&](FrameLaunch& F, const FrameRes& R) {
            F.SL.n = (int)nl;
            for (uint32_t l = 0; l < nl; l++) F.SL.l[l] = spec_level(R, l, R.stamp[l]);
            F.queue = R.pred_queue; F.qctl = R.pred_ctl; F.counters = count ? R.d_counters : nullptr;
            F.stamp_value = R.stamp_value; F.trace_flags = TRACE_PROBE_EMPTY;
        }), shared_device ? grid : full_device_grid(TraceBuild::dense), GRID_ID_MERGED, -1, TraceBuild::dense);
        for (uint32_t l = 0; l < nl; l++) {
            const LaunchArgs a = args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.L.pass = CLASSIFY_FIXUP; F.L.tag = (int)l;
                F.queue = R.queue[l]; F.qctl = R.d_qctl + 2 * l; F.counters = count ? R.d_counters + l : nullptr;
                F.need = R.need[l];
                F.stamp = R.stamp[l]; F.stamp_value = R.stamp_value; F.trace_flags = TRACE_PROBE_EMPTY;
                F.row_work = row_work(R, l);
            });
            classify(a, l, count, true).before(ev_level_begin(l)).after(ev_level_classified(l));
            trace(a, shared_device ? grid : full_device_grid(TraceBuild::latency), grid_id_level(l), (int)l, TraceBuild::latency);
        }
        first_normal = nl;
        return BHRAY_OK;
    }

    // the plain ladder: levels [first_normal, u0), one classify + one trace launch each
    void levels(uint32_t u0) {
        for (uint32_t l = first_normal; l < u0; l++) {
            const LaunchArgs a = args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.queue = R.queue[l]; F.qctl = R.d_qctl + 2 * l; F.counters = count ? R.d_counters + l : nullptr;
                F.row_work = row_work(R, l);
            });
            classify(a, l, count).before(ev_level_begin(l)).after(ev_level_classified(l));
            trace(a, grid, grid_id_level(l), (int)l, l + 1 < nl ? trace_build_of(c->coarse_build) : TraceBuild::ctx);
        }
    }

    // superset_levels = nu: the last nu levels traced in ONE launch over a conservative superset
    void superset(uint32_t nu, uint32_t u0) {
        // Superset speculation over the last nu levels: ONE trace launch instead of nu dependent ones.
        //  (1) tentative classification of levels u0..nl-1 in order: a pixel whose coarser inputs are known is classified exactly,
        //      a pixel with an input that is itself queued (PENDING) is queued conservatively -> one level-tagged queue;
        //  (2) one trace launch over it, each ray stored at its level's own place;
        //  (3) the levels are classified again, exactly, now that the coarser level is final: copy / interpolate are stored,
        //      pixels that need tracing keep what (2) wrote (the queued set is a superset of the needed one).
        // Same pixels as the plain ladder; the extra rays are the conservatively queued pixels that turn out to interpolate.
        // Queue control words of level u0 serve the merged queue; the trace is timed as level u0's.
        for (uint32_t l = u0; l < nl; l++) {
            Launch& Ln = classify(args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.L.pass = CLASSIFY_TENTATIVE; F.L.tag = (int)(l - u0); F.L.no_store = (l == nl - 1) ? 1 : 0;
                F.queue = R.super_queue; F.qctl = R.d_qctl + 2 * u0; F.counters = nullptr;
            }), l, false);
            if (l == u0) Ln.before(ev_level_begin(u0));
            if (l == nl - 1) Ln.after(ev_level_classified(u0));
        }
        trace(args_for(u0, [&](FrameLaunch& F, const FrameRes& R) {
            F.SL.n = (int)nu;
            for (uint32_t l = u0; l < nl; l++) F.SL.l[l - u0] = spec_level(R, l);
            F.queue = R.super_queue; F.qctl = R.d_qctl + 2 * u0; F.counters = count ? R.d_counters + u0 : nullptr;
        }), grid, GRID_ID_SUPERSET, (int)u0);
        for (uint32_t l = u0; l < nl; l++) {
            Launch& Ln = classify(args_for(l, [&](FrameLaunch& F, const FrameRes& R) {
                F.L.pass = CLASSIFY_KEEP;
                F.queue = nullptr; F.qctl = R.d_qctl + 2 * l; F.counters = count ? R.d_counters + l : nullptr;
            }), l, count);
            if (l > u0) Ln.before(ev_level_begin(l)).after(ev_level_classified(l), ev_level_traced(l));      // (level u0's: inside its trace interval)
        }
    }

    // step 3: the launches of the ctx's ladder mode, and their argument entries
    int build() {
        const uint32_t ns = c->cfg.speculative_levels;
        const bool temporal_mode = (c->cfg.flags & BHRAY_F_TEMPORAL) != 0;
        const uint32_t nu = temporal_mode ? 0 : c->cfg.superset_levels;
        const uint32_t u0 = nu ? nl - nu : nl;                     // first level of the superset group
        if (!c->levels[nl - 1].rows.empty()) {                     // a partition without rows has nothing to launch (then no level has rows)
            if (ns) speculative(ns);
            if (temporal_mode) { int rc = temporal(); if (rc) return rc; }
            levels(u0);
            if (nu) superset(nu, u0);
        }
        return overflow ? fail(c, BHRAY_E_STATE, "internal: argument block overflow") : BHRAY_OK;
    }

    // step 4: what every trace launch carries besides its plan's arguments - execution span, work counters, scheduling flags
    int decorate_traces() {
        if (timing && c->d_span) {                 // execution spans of this batch's trace launches (entry 0 of each launch's FrameLaunch array)
            int nt = 0;
            for (const Launch& Ln : seq) {
                if (Ln.kind != LaunchKind::trace || nt >= SPAN_MAX) continue;
                Ln.args.h[0].span = c->d_span + (ring * SPAN_MAX + (size_t)nt) * 2;
                nt++;
            }
            c->ring_spans[ring] = (uint8_t)nt;
            HIPCHK(c, hipMemsetAsync(c->d_span + ring * SPAN_MAX * 2, 0, (size_t)SPAN_MAX * 2 * sizeof(unsigned long long), st));
        } else {
            c->ring_spans[ring] = 0;
        }
        for (const Launch& Ln : seq) {             // every trace launch adds the steps its waves issue for a frame to that frame's work counters
            if (Ln.kind != LaunchKind::trace) continue;
            FrameLaunch* hl = Ln.args.h;
            for (uint32_t k = 0; k < nb; k++) hl[k].work = S.fr[k].d_work;
            // a whole frame, one frame per launch: thin shares are dealt strided (bhray_kernels.hip, thin_stride; TRACE_THIN_STRIDED)
            if (c->cfg.row_world <= 1 && nb == 1) hl[0].trace_flags |= TRACE_THIN_STRIDED;
            // the quad march (bhray_quad.inc) for launches whose queue turns out short: how many waves per SIMD it may use (TRACE_QUAD_WPS_*; 0 = off)
            // Measured (profiles/EXPERIMENTS.md R6.1): one wave per SIMD -21 % per launch (RK, a level-0-sized queue), two -10 %, three +10 %: a second wave on a
            // SIMD slows both, and from the third on a scalar wave with four times the rays is faster.  The Euler step has too little 3-vector work to gain at two.
            // Only for a host that renders one frame at a time (one frame per launch, at most two frame slots): beside other frames' waves on the same SIMDs
            // the quad march's shorter iteration is gone and its four lanes per ray cost throughput - a rank of an 8-way partition, batches of 5 frames: +3.5 %
            // per frame in the driver's blocks against -11-14 % one frame at a time (R6.1).  BHRAY_QUAD=n forces it for every latency-build launch.
            // ... and wave priority by predicted ray length (TRACE_WAVE_PRIO; BHRAY_WAVE_PRIO in bhray_kernels.hip) for a host with ONE frame slot: it shortens a lone frame's launches (S = 2 1.16 -> 1.13 ms,
            // S = 3 0.97 -> 0.95), but as soon as two frames overlap it costs - the drop-in shim with two frames in flight 0.816 -> 0.873 ms per frame, a saturated device 3.5 % (EXPERIMENTS.md R6.5)
            if (c->wave_prio >= 0 ? c->wave_prio != 0 : (nb == 1 && c->slots.size() <= 1)) for (uint32_t k = 0; k < nb; k++) hl[k].trace_flags |= TRACE_WAVE_PRIO;
            const int quad_wps = c->quad_wps >= 0 ? c->quad_wps : ((nb == 1 && c->slots.size() <= 2) ? (S.method == 0 ? 1 : 2) : 0);
            for (uint32_t k = 0; k < nb; k++) hl[k].trace_flags |= (quad_wps & TRACE_QUAD_WPS_MASK) << TRACE_QUAD_WPS_SHIFT;
        }
        return BHRAY_OK;
    }

    // step 5:
    // Trace grids by queue length.  Every ladder trace launch reports the rays its queues held (FrameLaunch::qlen -> S.h_qlen, one word per slot
    // position and launch); the next batch staged here gives the same launch enough blocks for that many rays plus a margin instead of the ctx's grid: a launch of the
    // coarse levels finds a few hundred waves' worth of rays, and every further wave of a full grid takes a wave slot, loads its arguments and fails an atomic on the
    // queue head only to leave.  Launches that RUN a dense build only (trace_resolve: a lensed-mesh launch, or a mesh launch of the literal / fma evaluations, asks for
    // one and gets the latency build, which sizes its thin shares, strided dealing and quad march from gridDim), not the temporal mode's
    // launches (their own rule, R4.10 / R4.12), not a counting ctx.  A word read here was written by the previous batch of this slot if that has run its trace launches
    // already, by the one before it otherwise (dev_render waited for the previous batch's upload, which follows the older batch's kernels in the stream): either is
    // an estimate, and a wrong estimate costs time only - persistent waves pull until the queues are exhausted, whatever the grid.  For the same reason the reset on
    // a change of kernel variant below is best effort: the slot's previous batch, of the old variant, may still be in flight and report behind it.
    void size_grids() {
        const bool report = !count && !(c->cfg.flags & BHRAY_F_TEMPORAL);
        if (S.qlen_method != S.method || S.qlen_models != S.models) {
            for (size_t i = 0; i < (size_t)c->batch * BHRAY_LEVEL_GRID_LAUNCHES; i++) S.h_qlen[i] = QLEN_NONE;
            S.qlen_method = S.method; S.qlen_models = S.models;
        }
        bhray_level_grid_info& G = S.grids;
        memset(&G, 0, sizeof G);
        for (int i = 0; i < BHRAY_LEVEL_GRID_LAUNCHES; i++) G.expected_rays[i] = BHRAY_LEVEL_GRID_NO_FEEDBACK;
        G.enabled = (report && c->level_grid) ? 1u : 0u; G.frames = nb; G.ctx_grid = (uint32_t)grid; G.dense = trace_resolve(ctx).dense ? 1u : 0u;
        for (Launch& Ln : seq) {
            if (Ln.kind != LaunchKind::trace || Ln.grid_id < 0) continue;
            const int unsized = Ln.blocks;
            uint64_t expected = BHRAY_LEVEL_GRID_NO_FEEDBACK;
            if (report) {
                uint64_t sum = 0; bool all = true;
                for (uint32_t k = 0; k < nb; k++) {
                    uint32_t* w = S.h_qlen + (size_t)k * BHRAY_LEVEL_GRID_LAUNCHES + (size_t)Ln.grid_id;
                    const uint32_t v = __atomic_load_n(w, __ATOMIC_RELAXED);
                    if (v == QLEN_NONE) all = false; else sum += v;
                    Ln.args.h[k].qlen = w;
                }
                if (all && c->level_grid && Ln.variant.dense) expected = sum;
            }
            if (expected != BHRAY_LEVEL_GRID_NO_FEEDBACK)
                Ln.blocks = (int)bhray_trace_grid_for(expected, nb, (uint32_t)Ln.blocks, c->level_grid_gen, c->level_grid_margin, c->level_grid_floor);
            G.expected_rays[Ln.grid_id] = expected; G.blocks[Ln.grid_id] = (uint32_t)Ln.blocks;
            c->grid_launches++; c->grid_blocks += (uint64_t)Ln.blocks; if (Ln.blocks >= unsized) c->grid_ceiling_launches++;
        }
    }

    // step 6: the argument block, then the launches in order
    int enqueue() {
        const FrameParams* dP = (const FrameParams*)S.d_args;
        HIPCHK(c, launch_upload(S.h_args, S.d_args, (args_used + 15) / 16, S.d_qctl, (size_t)nb * BHRAY_QCTL_WORDS, st));   // + queue control reset
        HIPCHK(c, hipEventRecord(S.uploaded, st));
        if (count) HIPCHK(c, hipMemsetAsync(S.d_counters, 0, (size_t)nb * BHRAY_MAX_LEVELS * sizeof(Counters64), st));
        if (count) for (uint32_t k = 0; k < nb; k++) if (S.fr[k].d_row_work) HIPCHK(c, hipMemsetAsync(S.fr[k].d_row_work, 0, c->row_work_off[nl] * sizeof(unsigned long long), st));
        hipEvent_t* fev = timing ? batch_events(c, ring) : nullptr;
        if (timing) { c->sky_recorded[ring] = 0; c->ring_frames[ring] = (uint8_t)nb; c->ring_own_trace[ring] = (uint8_t)own_trace; }
        for (const Launch& Ln : seq) {
            if (timing) for (int e : Ln.ev_before) if (e >= 0) HIPCHK(c, hipEventRecord(fev[e], st));
            if (Ln.kind == LaunchKind::predict) HIPCHK(c, launch_predict(dP, Ln.args.d, (int)nb, Ln.levels, Ln.blocks, st));
            else if (Ln.kind == LaunchKind::classify) HIPCHK(c, launch_classify(dP, Ln.args.d, (int)nb, Ln.blocks, Ln.count, Ln.fixup, st));
            else {
                HIPCHK(c, launch_trace(dP, Ln.args.d, (int)nb, Ln.variant, c->d_err, Ln.blocks, st));
                if (Ln.variant.origin) c->origin_launches++; else c->general_launches++;
            }
            if (timing) for (int e : Ln.ev_after) if (e >= 0) HIPCHK(c, hipEventRecord(fev[e], st));
        }
        HIPCHK(c, hipEventRecord(S.done, st));
        return BHRAY_OK;
    }
};

// step 1: the trace build this batch's launches ask for, where the plan names no other
TraceVariant choose_build(bhray_dev* c, const Slot& S, uint32_t nb) {
    // Register budget of the no-mesh trace kernel (bhray_kernels.hip): the dense build when the device is saturated with
    // rays - at least ~4 whole frames' worth in flight (slots x frames per batch / row partitions) - otherwise the latency
    // build (measured on MI355X: 1920x1080, 16 slots: 4830 vs 4160 Mrays/s; 1/8 row tile, 16 slots x 8 frames: 0.070 vs
    // 0.080 ms per frame; one slot: the latency build is 7-15 % faster per launch).
    // ... with four or more row partitions a rank's launches are small and a timed block may hold only a few batches: there the count is
    // the batches IN FLIGHT when this one is launched (completed ones are retired oldest-first, one or two event queries per launch),
    // dense from 8 partitions' worth on (emulated ranks, 20-frame blocks: N = 8 0.1018 -> 0.0992 ms per frame, N = 4 0.1469 -> 0.1403;
    // 400-frame blocks unchanged; a whole frame per GPU loses 1-2 % with it: profiles/EXPERIMENTS.md R3.11).
    // ... and what counts is rays, not frames: a partition of a 3840x2160 frame holds four times the rays of the same partition of a
    // 1920x1080 one, so the frames in flight are weighted by the frame's pixels against 1920x1080 (the size the thresholds were measured
    // at; 3840x2160 over 8 partitions, 20-frame blocks: the dense build 0.2499 / 0.2407 ms per frame at 4 / 7 frames per batch against
    // 0.2614 / 0.2550 for the latency build - profiles/r04_emu_knobs.txt).
    const int dyn = c->dynamic_dense >= 0 ? c->dynamic_dense : (c->cfg.row_world >= 4 ? 8 : 0);
    size_t in_flight = c->slots.size();
    if (dyn > 0) {
        while (c->retired < c->batch_counter) {
            const Slot& O = c->slots[(size_t)(c->retired % c->slots.size())];
            if (O.batch_id == c->retired && hipEventQuery(O.done) != hipSuccess) break;
            c->retired++;
        }
        in_flight = (size_t)(c->batch_counter - c->retired) + 1;
    }
    // A launch that by itself holds 2.5 frames' worth of rays is dense whatever else is in flight (the first batches of a short block).
    const double weight = std::max(1.0, (double)c->cfg.frame_w * (double)c->cfg.frame_h / (1920.0 * 1080.0)) / (double)c->cfg.row_world;   // 1920x1080 frames' worth per frame of this partition
    const bool dense = c->dense_override >= 0 ? c->dense_override != 0
                                              : ((double)nb * weight >= 2.5 || (double)(in_flight * (size_t)c->batch) * weight >= (double)(dyn > 0 ? dyn : 4));
    const int literal = (c->cfg.flags & BHRAY_F_LITERAL) ? 1 : ((c->cfg.flags & BHRAY_F_EVAL_FMA) ? 2 : 0);   // the integrator's evaluation (TraceVariant::eval)
    // The hole at the scene's origin - the three position words of EVERY frame staged in this batch are zero bits (a -0 is not: x - (-0) is not x for x = -0) - selects the ORIGIN
    // builds of the trace kernels (bhray_kernels.hip: no position - bpos in the march) for every trace launch of the batch and for the occupancy query that sizes their grids.
    // Per batch, from the uniform words staged with each frame: a scene whose hole moves changes builds from one batch to the next, with the same pixels.
    bool origin = c->origin_kernel != 0;
    for (uint32_t k = 0; k < nb && origin; k++) {
        uint32_t w[3];
        memcpy(w, ((const FrameParams*)S.h_args)[k].bh, sizeof w);
        origin = (w[0] | w[1] | w[2]) == 0u;
    }
    return {S.method, S.models, (c->cfg.flags & BHRAY_F_COUNTERS) != 0, dense, literal, origin};
}

// step 2: the persistent blocks of a trace launch of that build
int choose_grid(const bhray_dev* c, const TraceVariant& ctx) {
    // Persistent trace grid: (resident blocks per CU) x CUs.  With several batches in flight each launch takes only
    // half of the block slots: the kernels of the other batches fill the rest, and a wave of a half-size grid pulls
    // more than one load of rays, so the refill keeps its lanes busy (+4 % at 16 slots).
    int bpc = trace_blocks_per_cu(ctx);
    if (c->slots.size() > 1 && bpc > 1) bpc = bpc > 4 ? 2 : (bpc / 2 > 1 ? bpc / 2 : 1);     // measured: 2 blocks per CU is best at 8-16 slots
    if (c->bpc_override > 0) bpc = c->bpc_override;
    int grid = c->num_cus * bpc;
    // ... and one and a half for the Euler kernels (their steps are short: a block's share of a queue is used up sooner, and a smaller grid leaves the later launches'
    // blocks room beside it): 512 -> 384 blocks at 22 slots +1.5 % (20- and 400-frame blocks), with the mesh +2.4-3 %, a rank of 8 0 / +2 %; the RK kernels: nothing
    // (profiles/r05_ab_euler_grid.txt, EXPERIMENTS.md R5.9)
    if (ctx.method == 0 && c->slots.size() >= 8 && bpc == 2 && c->bpc_override <= 0) grid = c->num_cus * 3 / 2;      // (measured at 22 slots only: from 8 slots on)
    if (c->grid_override > 0) grid = c->grid_override;
    return grid;
}

// Enqueues every launch of the batch staged in the current slot: one argument block (FrameParams + per-launch FrameLaunch
// arrays) copied to the device, then the same launch sequence a single frame needs, each launch covering all staged frames.
int launch_batch(bhray_dev* c) {
    Slot& S = c->slots[(size_t)(c->batch_counter % c->slots.size())];
    const uint32_t nb = S.pending;
    if (nb == 0) return BHRAY_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // BHRAY_F_TIMING_SPARSE: events around the launches of every 4th batch only (every recorded event is a packet in the stream's
    // queue: 12 per frame cost a saturated device 1.6 %)
    const bool sparse = (c->cfg.flags & BHRAY_F_TIMING_SPARSE) != 0;
    const bool timing = (c->cfg.flags & (BHRAY_F_TIMING | BHRAY_F_TIMING_SPARSE)) != 0 && (!sparse || (c->batch_counter & 3u) == 0);
    const size_t ring = (size_t)(c->batch_counter % BHRAY_TIMING_RING);
    if ((c->cfg.flags & (BHRAY_F_TIMING | BHRAY_F_TIMING_SPARSE)) != 0 && !timing) { c->ring_frames[ring] = 0; c->sky_recorded[ring] = 0; }   // this batch carries no events
    const TraceVariant ctx = choose_build(c, S, nb);
    BatchPlan plan{c, S, nb, c->cfg.levels, ctx, choose_grid(c, ctx), timing, ring, S.stream, (size_t)c->batch * sizeof(FrameParams)};
    { int rc = plan.build(); if (rc) return rc; }
    { int rc = plan.decorate_traces(); if (rc) return rc; }
    plan.size_grids();
    S.launched_frames = nb;
    { int rc = plan.enqueue(); if (rc) return rc; }
    S.used = true;
    S.batch_id = c->batch_counter;
    S.pending = 0;
    c->launched_slot = (int)(c->batch_counter % c->slots.size());
    c->launched_frames = nb;
    c->batch_counter++;
    return BHRAY_OK;
}

// kernel variant the current uniforms and scene need (same rule as derive_frame: a mesh only when one is usable and visible)
void frame_variant(const bhray_dev* c, int& method, int& models) {
    method = c->det.integration_method != 0 ? 1 : 0;
    int mc = c->det.model_count; if (mc < 0) mc = 0; if (mc > BHRAY_MAX_MODELS) mc = BHRAY_MAX_MODELS;
    models = 0;
    for (int i = 0; i < mc; i++) {
        const ModelStore& m = c->models[i];
        if (m.loaded && m.triangle_count > 0 && m.visible != 0) models = c->mesh_lensing ? 2 : 1;
    }
}
}  // namespace

int dev_flush(bhray_dev* c) {
    if (!c) return BHRAY_E_INVALID;
    return launch_batch(c);
}

int dev_render(bhray_dev* c) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->have_uniforms) return fail(c, BHRAY_E_STATE, "dev_set_uniforms has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    FrameParams P;
    derive_frame(c, P);
    const int models = P.model_count > 0 ? (c->mesh_lensing ? 2 : 1) : 0;      // (frame_variant's rule; no usable visible model: the no-mesh kernels, lensing or not)
    {   // a batch runs one kernel variant: launch what is staged if this frame needs another
        Slot& S0 = c->slots[(size_t)(c->batch_counter % c->slots.size())];
        if (S0.pending > 0 && (S0.method != P.method || S0.models != models)) { int rc = launch_batch(c); if (rc) return rc; }
    }
    const int si = (int)(c->batch_counter % c->slots.size());
    Slot& S = c->slots[(size_t)si];
    if (S.pending == 0) {
        // the slot's previous argument block must have reached the device before the pinned copy is rewritten
        if (S.used && hipEventQuery(S.uploaded) != hipSuccess) HIPCHK(c, hipEventSynchronize(S.uploaded));
        S.method = P.method; S.models = models;
    }
    for (hipEvent_t ev : c->waits) HIPCHK(c, hipStreamWaitEvent(S.stream, ev, 0));
    c->waits.clear();
    const uint32_t k = S.pending;
    FrameRes& R = S.fr[k];
    ((FrameParams*)S.h_args)[k] = P;
    R.out = c->bound_out ? c->bound_out : R.own_out;
    c->bound_out = nullptr;                                   // a binding applies to one frame
    if (!R.out && c->out_bytes) return fail(c, BHRAY_E_STATE, "internal: no output bound for this frame");
    R.frame_id = c->frame_counter;
    {   // the level row the hole projects to (create_ray, ray.wgsl:269-285, inverted): its rows are classified first
        const F3 d = ld3(P.bh) - ld3(P.cam), ff = ld3(P.fwd_ff);
        const float along = dot(d, ff) / dot(ff, ff);
        float frac = 0.5f;
        if (along > 0.0f) {
            const Level& Ll = c->levels[c->cfg.levels - 1];
            const float sm = (float)std::min(Ll.w - 1, Ll.h - 1);
            const float posy = dot(d, ld3(P.up)) / along;
            frac = (posy * sm * 0.5f + (float)(Ll.h - 1) * 0.5f) / (float)std::max(1, Ll.h - 1);
        }
        if (!(frac >= 0.0f)) frac = 0.0f;
        if (frac > 1.0f) frac = 1.0f;
        // ... when few frames are in flight (a host that presents every frame: a launch then lasts as long as its last rays - one frame at a time
        // 1.136 -> 1.087 ms, the drop-in shim with 2 frames in flight 2 515 -> 2 618 Mrays/s); with many frames in flight the launches overlap each
        // other's tails and the ascending order keeps its locality (4K / Euler -1 % with the ordering: EXPERIMENTS R4.16)
        R.row_variant = (BHRAY_ROW_VARIANTS >= 2 && c->slots.size() <= 4) ? (int)lrintf(frac * (float)(BHRAY_ROW_VARIANTS - 1)) : -1;
    }
    S.pending = k + 1;
    c->last_slot = si; c->last_sub = (int)k;
    c->rendered = true;
    c->frame_counter++;
    if (S.pending == c->batch) return launch_batch(c);
    return BHRAY_OK;
}

int dev_sync(bhray_dev* c) {
    if (!c) return BHRAY_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    HIPCHK(c, sync_all(c));
    if (c->rendered || c->q_used) {
        int e = 0;
        HIPCHK(c, hipMemcpy(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost));
        if (e != 0) {
            HIPCHK(c, hipMemset(c->d_err, 0, sizeof(int)));
            return fail(c, e, "kernel reported: %s", bhray_strerror(e));
        }
    }
    return BHRAY_OK;
}

uint32_t dev_local_rows(const bhray_dev* c) { return c ? (uint32_t)c->local_rows.size() : 0; }

int dev_local_row_index(const bhray_dev* c, uint32_t i, uint32_t* frame_row) {
    if (!c || !frame_row || i >= c->local_rows.size()) return BHRAY_E_INVALID;
    *frame_row = c->local_rows[i];
    return BHRAY_OK;
}

// ---- the three images of the most recently staged frame (bhray::ImageKind) ---------------------------------------
namespace {
// the display pass (bhray_post.hip) and its image need the whole frame on this engine
int display_whole_frame(bhray_dev* c) {
    if (c->local_rows.size() != (size_t)c->cfg.frame_h)
        return fail(c, BHRAY_E_STATE, "the display pass needs the whole frame: this ctx renders %zu of %u rows (BHRAY_GATHER_NONE)", c->local_rows.size(), c->cfg.frame_h);
    if (display_scratch_bytes(c->cfg.frame_w, c->cfg.frame_h) == 0) return fail(c, BHRAY_E_INVALID, "the display pass needs a frame of at least 32 x 32 pixels");
    return BHRAY_OK;
}

// "Resolved for this frame", written here and nowhere else: a slot position is reused, so an image belongs to the frame whose id it was stamped
// with by its resolve pass, and an older frame's image is stale.  (The ray pass writes the hdr frame itself: nothing to resolve.)
bool resolved(const FrameRes& R, ImageKind kind) {
    if (kind == IMAGE_SKY) return R.sky_out && R.sky_frame_id == R.frame_id;
    if (kind == IMAGE_DISPLAY) return R.disp_out && R.disp_frame_id == R.frame_id;
    return true;
}

// Image `kind` of the most recently staged frame: its description, or the refusal.  The checks that every access form shares, in their one
// order: a frame exists (need_frame - the hdr buffer exists from dev_create on, so a pointer to it and the blocking read never asked), this
// engine holds the image, the image was resolved for THIS frame.
// img->rows == 0: this partition owns no rows - nothing to copy and nothing to have resolved; img->stream is still the frame's stream.
int last_image(bhray_dev* c, ImageKind kind, bool need_frame, FrameImage* img) {
    *img = FrameImage{};
    if (need_frame && !c->rendered) return fail(c, BHRAY_E_STATE, "nothing rendered yet");
    Slot& S = c->slots[(size_t)c->last_slot];
    const FrameRes& R = S.fr[(size_t)c->last_sub];
    img->stream = S.stream;
    if (kind == IMAGE_HDR) { img->src = R.out; img->render_target = true; }
    if (kind == IMAGE_DISPLAY) { int rc = display_whole_frame(c); if (rc) return rc; }
    else if (c->local_rows.empty()) return BHRAY_OK;
    if (!resolved(R, kind)) return fail(c, BHRAY_E_STATE, "%s has not been called for this frame", kind == IMAGE_SKY ? "dev_resolve_sky" : "bhray_resolve_display");
    if (kind == IMAGE_SKY) img->src = R.sky_out;
    if (kind == IMAGE_DISPLAY) img->src = R.disp_out;
    img->rows = c->local_rows.size();
    img->row_bytes = (size_t)c->cfg.frame_w * (kind == IMAGE_HDR ? sizeof(float4) : kind == IMAGE_SKY ? sizeof(uint2) : sizeof(uint32_t));
    return BHRAY_OK;
}
}  // namespace

int dev_read(bhray_dev* c, ImageKind kind, void* dst, size_t pitch) {
    if (!c) return BHRAY_E_INVALID;
    FrameImage img;
    { int rc = last_image(c, kind, false, &img); if (rc) return rc; }
    if (img.rows && !img.fits(dst, pitch)) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    { int rc = dev_sync(c); if (rc) return rc; }
    if (img.rows) HIPCHK(c, img.copy_to(dst, pitch, false));
    return BHRAY_OK;
}

// Asynchronous hand-off of the most recently enqueued frame to host memory (a consumer on another device: the wgpu texture the
// reference's SkyPipeline samples, ray_pipeline.rs:297-299, mod.rs:215).  The copy (SDMA: no CU time, 55.7 GB/s into pinned memory
// on this box) is enqueued ON THE FRAME'S OWN SLOT STREAM, behind its kernels and resolve passes; the call returns at once and the other
// slots' frames render while it runs.  (First version: dedicated copy streams ordered by events both ways - ROCm 7.2 then ran copies and
// kernels strictly one after the other, 1.22 ms per 1080p frame; in stream order 0.62 ms, which is the link rate: profiles/EXPERIMENTS.md.)
// `dst` should be pinned (bhray_host_alloc / hipHostRegister): a pageable destination makes the runtime stage the copy.
// Every refusal - no frame, no resolve for this frame, an unusable destination - comes BEFORE anything is launched and before the ring is
// touched: a misuse must not flush a partly filled batch on its way to the error, and consumes no ticket.  (The hdr and sky reads used to
// refuse a bad destination behind the flush; the display read already did it this way.)
int dev_read_async(bhray_dev* c, ImageKind kind, void* dst, size_t pitch, uint64_t* ticket) {
    if (!c || !ticket) return BHRAY_E_INVALID;
    FrameImage img;
    { int rc = last_image(c, kind, true, &img); if (rc) return rc; }
    if (img.rows && !img.fits(dst, pitch)) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }          // (a resolve launched the frame's batch: nothing is pending then)
    hipEvent_t ev;
    HIPCHK(c, c->reads.acquire(&ev));
    if (img.rows) HIPCHK(c, img.copy_to(dst, pitch, true));
    HIPCHK(c, hipEventRecord(ev, img.stream));
    HIPCHK(c, hipEventRecord(c->slots[(size_t)c->last_slot].done, img.stream));   // whatever is ordered behind this slot's frame is ordered behind its copy too
    *ticket = c->reads.commit();
    return BHRAY_OK;
}

int dev_device_ptr(bhray_dev* c, ImageKind kind, void** p, size_t* bytes) {
    if (!c || !p) return BHRAY_E_INVALID;
    *p = nullptr;
    FrameImage img;
    { int rc = last_image(c, kind, false, &img); if (rc) return rc; }
    *p = (void*)img.src;
    if (bytes) *bytes = img.rows * img.row_bytes;
    return BHRAY_OK;
}

int dev_wait_read(bhray_dev* c, uint64_t ticket) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->reads.known(ticket)) return fail(c, BHRAY_E_INVALID, "unknown read ticket");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->reads.wait(ticket));
    return BHRAY_OK;
}

int dev_read_level(bhray_dev* c, uint32_t level, float* dst, size_t pitch) {
    if (!c) return BHRAY_E_INVALID;
    if (level >= c->cfg.levels) return fail(c, BHRAY_E_INVALID, "level out of range");
    const Level& L = c->levels[level];
    const size_t rowb = (size_t)L.w * sizeof(float4);
    if (!dst || pitch < rowb) return fail(c, BHRAY_E_INVALID, "bad destination / pitch");
    int rc = dev_sync(c);
    if (rc) return rc;
    if (level + 1 < c->cfg.levels) {
        HIPCHK(c, hipMemcpy2D(dst, pitch, c->slots[(size_t)c->last_slot].fr[(size_t)c->last_sub].level_out[level], rowb, rowb, (size_t)L.h, hipMemcpyDeviceToHost));
        return BHRAY_OK;
    }
    // last level: scatter the packed window back into a NaN canvas of the full level size
    for (int y = 0; y < L.h; y++) memset((uint8_t*)dst + (size_t)y * pitch, 0xFF, rowb);
    const size_t frb = (size_t)c->cfg.frame_w * sizeof(float4);
    std::vector<uint8_t> tmp(c->local_rows.size() * frb);
    if (!tmp.empty()) HIPCHK(c, hipMemcpy(tmp.data(), c->slots[(size_t)c->last_slot].fr[(size_t)c->last_sub].out, tmp.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < c->local_rows.size(); i++) {
        uint8_t* row = (uint8_t*)dst + (size_t)(c->cfg.crop_y + c->local_rows[i]) * pitch + (size_t)c->cfg.crop_x * sizeof(float4);
        memcpy(row, tmp.data() + i * frb, frb);
    }
    return BHRAY_OK;
}

int dev_bind_output(bhray_dev* c, void* p, size_t bytes) {
    if (!c) return BHRAY_E_INVALID;
    if (!p) { c->bound_out = nullptr; return BHRAY_OK; }
    if (bytes < c->out_bytes) return fail(c, BHRAY_E_INVALID, "output binding needs %zu bytes", c->out_bytes);
    if (((uintptr_t)p & 15u) != 0) return fail(c, BHRAY_E_INVALID, "output binding must be 16-byte aligned");
    c->bound_out = (float4*)p;
    return BHRAY_OK;
}

int dev_resolve_sky(bhray_dev* c) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->rendered) return fail(c, BHRAY_E_STATE, "nothing rendered yet");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    Slot& S = c->slots[(size_t)c->last_slot];
    FrameRes& R = S.fr[(size_t)c->last_sub];
    const size_t npix = c->local_rows.size() * (size_t)c->cfg.frame_w;
    if (!R.sky_out && npix) HIPCHK(c, hipMalloc(&R.sky_out, npix * sizeof(uint2)));
    TexDev sky; sky.rgba = c->tex[BHRAY_TEX_SKY]; sky.w = c->tex_w[BHRAY_TEX_SKY]; sky.h = c->tex_h[BHRAY_TEX_SKY];
    const bool timing = (c->cfg.flags & BHRAY_F_TIMING) != 0;
    const size_t ring = (size_t)(S.batch_id % BHRAY_TIMING_RING);
    hipEvent_t* ev = timing ? batch_events(c, ring) : nullptr;
    if (timing) HIPCHK(c, hipEventRecord(ev[ev_sky_begin(c->cfg.levels)], S.stream));
    if (c->sky_filter != 0 && c->local_rows.size() != (size_t)c->cfg.frame_h) return fail(c, BHRAY_E_STATE, "the sky filter needs the whole frame on this engine");
    if (c->sky_filter == 0) HIPCHK(c, launch_sky(sky, R.out, R.sky_out, npix, S.stream));
    else HIPCHK(c, launch_sky_filter(sky, c->pyr, R.out, R.sky_out, c->cfg.frame_w, c->cfg.frame_h, S.stream));     // the whole frame: dev_set_sky_filter refuses a partition
    if (c->stars.stars) {                                            // point stars: added into the image the sky kernel has just written, the whole frame
        if (c->local_rows.size() != (size_t)c->cfg.frame_h) return fail(c, BHRAY_E_STATE, "point stars need the whole frame on this engine");
        HIPCHK(c, launch_stars(c->stars, R.out, R.sky_out, c->cfg.frame_w, c->cfg.frame_h, S.stream));
    }
    R.sky_frame_id = R.frame_id;
    if (timing) { HIPCHK(c, hipEventRecord(ev[ev_sky_end(c->cfg.levels)], S.stream)); c->sky_recorded[ring] = 1; }
    HIPCHK(c, hipEventRecord(S.done, S.stream));
    return BHRAY_OK;
}

// the display pass (bhray_post.hip) behind the last frame and its sky image
int dev_resolve_display(bhray_dev* c, const bhray_fxaa_details* fx, const bhray_mix_details* mx) {
    if (!c || !fx || !mx) return BHRAY_E_INVALID;
    if (!c->rendered) return fail(c, BHRAY_E_STATE, "nothing rendered yet");
    { int rc = display_whole_frame(c); if (rc) return rc; }
    Slot& S = c->slots[(size_t)c->last_slot];
    FrameRes& R = S.fr[(size_t)c->last_sub];
    if (!resolved(R, IMAGE_SKY)) { int rc = dev_resolve_sky(c); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    const size_t npix = (size_t)c->cfg.frame_w * c->cfg.frame_h;
    if (!S.post_scratch) HIPCHK(c, hipMalloc(&S.post_scratch, display_scratch_bytes(c->cfg.frame_w, c->cfg.frame_h)));
    if (!R.disp_out) HIPCHK(c, hipMalloc(&R.disp_out, npix * sizeof(uint32_t)));
    HIPCHK(c, launch_display(R.sky_out, S.post_scratch, R.disp_out, c->cfg.frame_w, c->cfg.frame_h, *fx, *mx, S.stream));
    R.disp_frame_id = R.frame_id;
    HIPCHK(c, hipEventRecord(S.done, S.stream));
    return BHRAY_OK;
}

// the display pass of a gathered frame on the root (bhray_group.hip): sky image -> RGBA8 on the caller's stream
int dev_launch_display(bhray_dev* c, const void* sky, void* scratch, void* dst, const bhray_fxaa_details* fx, const bhray_mix_details* mx, hipStream_t stream) {
    if (!c || !fx || !mx) return BHRAY_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_display((const uint2*)sky, (uint2*)scratch, (uint32_t*)dst, c->cfg.frame_w, c->cfg.frame_h, *fx, *mx, stream));
    return BHRAY_OK;
}

int dev_wait_event(bhray_dev* c, hipEvent_t ev) {
    if (!c || !ev) return BHRAY_E_INVALID;
    c->waits.push_back(ev);
    return BHRAY_OK;
}

int dev_device(const bhray_dev* c) { return c ? c->device : -1; }

int dev_next_position(bhray_dev* c, int* slot, uint32_t* sub) {
    if (!c || !slot || !sub) return BHRAY_E_INVALID;
    Slot& S0 = c->slots[(size_t)(c->batch_counter % c->slots.size())];
    if (S0.pending > 0) {
        int method, models;
        frame_variant(c, method, models);
        if (S0.method != method || S0.models != models) { int rc = launch_batch(c); if (rc) return rc; }
    }
    *slot = (int)(c->batch_counter % c->slots.size());
    *sub = c->slots[(size_t)*slot].pending;
    return BHRAY_OK;
}

void dev_peek_position(const bhray_dev* c, uint64_t* batch_counter, uint32_t* pending, int* method, int* models) {
    const Slot& S = c->slots[(size_t)(c->batch_counter % c->slots.size())];
    *batch_counter = c->batch_counter; *pending = S.pending; *method = S.method; *models = S.models;
}

bool dev_take_launched(bhray_dev* c, int* slot, uint32_t* frames) {
    if (!c || c->launched_slot < 0) return false;
    if (slot) *slot = c->launched_slot;
    if (frames) *frames = c->launched_frames;
    c->launched_slot = -1; c->launched_frames = 0;
    return true;
}

int* dev_err_flag(bhray_dev* c) { return c->d_err; }
hipStream_t dev_slot_stream(bhray_dev* c, int slot) { return c->slots[(size_t)slot].stream; }
hipEvent_t dev_slot_done(bhray_dev* c, int slot) { return c->slots[(size_t)slot].done; }

int dev_launch_sky(bhray_dev* c, const void* src, void* dst, size_t npix, hipStream_t stream) {
    if (!c) return BHRAY_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TexDev sky; sky.rgba = c->tex[BHRAY_TEX_SKY]; sky.w = c->tex_w[BHRAY_TEX_SKY]; sky.h = c->tex_h[BHRAY_TEX_SKY];
    HIPCHK(c, launch_sky(sky, (const float4*)src, (uint2*)dst, npix, stream));
    return BHRAY_OK;
}

int dev_next_stream(bhray_dev* c, void** s) {
    if (!c || !s) return BHRAY_E_INVALID;
    *s = (void*)c->slots[(size_t)(c->batch_counter % c->slots.size())].stream;
    return BHRAY_OK;
}

int dev_signal_stream(bhray_dev* c, void* s) {
    if (!c) return BHRAY_E_INVALID;
    if (!c->rendered) return BHRAY_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = launch_batch(c); if (rc) return rc; }
    HIPCHK(c, hipStreamWaitEvent((hipStream_t)s, c->slots[(size_t)c->last_slot].done, 0));
    return BHRAY_OK;
}

int dev_get_level_grids(bhray_dev* c, uint32_t slot, bhray_level_grid_info* out) {
    if (!c || !out) return BHRAY_E_INVALID;
    if (slot >= c->slots.size()) return fail(c, BHRAY_E_INVALID, "slot %u of %zu", slot, c->slots.size());
    *out = c->slots[slot].grids;
    if (out->frames == 0) {                              // nothing launched from this slot yet
        for (int i = 0; i < BHRAY_LEVEL_GRID_LAUNCHES; i++) out->expected_rays[i] = BHRAY_LEVEL_GRID_NO_FEEDBACK;
        out->enabled = (c->level_grid && !(c->cfg.flags & (BHRAY_F_COUNTERS | BHRAY_F_TEMPORAL))) ? 1u : 0u;
    }
    out->total_launches = c->grid_launches; out->total_blocks = c->grid_blocks; out->total_ceiling_launches = c->grid_ceiling_launches;
    return BHRAY_OK;
}

int dev_get_trace_builds(bhray_dev* c, uint64_t launches[2]) {
    if (!c || !launches) return BHRAY_E_INVALID;
    launches[0] = c->origin_launches; launches[1] = c->general_launches;
    return BHRAY_OK;
}

int dev_selftest(bhray_dev* c, uint64_t mismatches[3]) {
    if (!c || !mismatches) return BHRAY_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    HIPCHK(c, hipMalloc(&d, 24));
    hipError_t e = hipMemset(d, 0, 24);
    if (e == hipSuccess) e = launch_selftest(d, nullptr);
    unsigned long long h[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, BHRAY_E_HIP, "selftest: %s", hipGetErrorString(e));
    mismatches[0] = h[0]; mismatches[1] = h[1]; mismatches[2] = h[2];
    return BHRAY_OK;
}

int dev_get_level_counters(bhray_dev* c, uint32_t level, bhray_counters* out) {
    if (!c || !out) return BHRAY_E_INVALID;
    if (!(c->cfg.flags & BHRAY_F_COUNTERS)) return fail(c, BHRAY_E_STATE, "ctx created without BHRAY_F_COUNTERS");
    if (level >= c->cfg.levels) return fail(c, BHRAY_E_INVALID, "level out of range");
    int rc = dev_sync(c);
    if (rc) return rc;
    static_assert(sizeof(bhray_counters) == 13 * sizeof(unsigned long long) && sizeof(Counters64) == 16 * sizeof(unsigned long long), "counter layout");
    HIPCHK(c, hipMemcpy(out, c->slots[(size_t)c->last_slot].fr[(size_t)c->last_sub].d_counters + level, sizeof(bhray_counters), hipMemcpyDeviceToHost));
    return BHRAY_OK;
}

// The RK error-estimate bound's counters of the last render (Counters64::v[13..15], summed over the levels): wave-steps, wave-steps whose active lanes all passed, violations
int dev_get_err_skip(bhray_dev* c, uint64_t out[3]) {
    if (!c || !out) return BHRAY_E_INVALID;
    if (!(c->cfg.flags & BHRAY_F_COUNTERS)) return fail(c, BHRAY_E_STATE, "ctx created without BHRAY_F_COUNTERS");
    int rc = dev_sync(c);
    if (rc) return rc;
    Counters64 t[BHRAY_MAX_LEVELS];
    HIPCHK(c, hipMemcpy(t, c->slots[(size_t)c->last_slot].fr[(size_t)c->last_sub].d_counters, (size_t)c->cfg.levels * sizeof(Counters64), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = 0;
    for (uint32_t l = 0; l < c->cfg.levels; l++) for (int k = 0; k < 3; k++) out[k] += t[l].v[13 + k];
    return BHRAY_OK;
}

int dev_add_row_work(bhray_dev* c, uint32_t level, uint64_t* acc, uint32_t n) {
    if (!c || !acc) return BHRAY_E_INVALID;
    if (!(c->cfg.flags & BHRAY_F_COUNTERS)) return fail(c, BHRAY_E_STATE, "ctx created without BHRAY_F_COUNTERS");
    if (level >= c->cfg.levels || n != c->cfg.level_h[level]) return fail(c, BHRAY_E_INVALID, "level out of range, or n is not the level's height");
    int rc = dev_sync(c);
    if (rc) return rc;
    const FrameRes& R = c->slots[(size_t)c->last_slot].fr[(size_t)c->last_sub];
    std::vector<unsigned long long> tmp(n);
    HIPCHK(c, hipMemcpy(tmp.data(), R.d_row_work + c->row_work_off[level], (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (uint32_t y = 0; y < n; y++) acc[y] += tmp[y];
    return BHRAY_OK;
}

// What the frames of the batches still held by the slots cost this engine: integrator steps issued by its trace waves (FrameLaunch::work),
// mean per frame, and the pixels its classify launches visit per frame (an HBM-bound pass: its cost goes with the pixels).
int dev_get_work(bhray_dev* c, double* wave_steps_per_frame, double* classify_pixels_per_frame, uint32_t* frames, int* method) {
    if (!c || !wave_steps_per_frame || !classify_pixels_per_frame || !frames || !method) return BHRAY_E_INVALID;
    int rc = dev_sync(c);
    if (rc) return rc;
    std::vector<uint32_t> tmp((size_t)c->batch * BHRAY_QCTL_WORDS);
    double sum = 0.0; uint32_t n = 0;
    for (const Slot& S : c->slots) {
        if (!S.used || S.launched_frames == 0) continue;
        HIPCHK(c, hipMemcpy(tmp.data(), S.d_qctl, (size_t)S.launched_frames * BHRAY_QCTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < S.launched_frames; k++) {
            unsigned long long w[BHRAY_WORK_WORDS];
            memcpy(w, tmp.data() + (size_t)k * BHRAY_QCTL_WORDS + 2 * BHRAY_MAX_LEVELS, sizeof w);
            for (unsigned long long v : w) sum += (double)v;
            n++;
        }
    }
    double px = 0.0;
    for (const Level& L : c->levels) px += (double)L.queue_cap;
    *wave_steps_per_frame = n ? sum / (double)n : 0.0;
    *classify_pixels_per_frame = px;
    *frames = n;
    *method = c->det.integration_method != 0 ? 1 : 0;
    return BHRAY_OK;
}

int dev_get_counters(bhray_dev* c, bhray_counters* out) {
    if (!c || !out) return BHRAY_E_INVALID;
    memset(out, 0, sizeof *out);
    for (uint32_t l = 0; l < c->cfg.levels; l++) {
        bhray_counters t;
        int rc = dev_get_level_counters(c, l, &t);
        if (rc) return rc;
        const uint64_t* a = (const uint64_t*)&t; uint64_t* b = (uint64_t*)out;
        for (size_t k = 0; k < sizeof(bhray_counters) / 8; k++) { if (k == 12) b[k] = a[k] > b[k] ? a[k] : b[k]; else b[k] += a[k]; }   // [12] max_ray_iterations
    }
    return BHRAY_OK;
}

int dev_get_timing(bhray_dev* c, bhray_timing* out) {
    if (!c || !out) return BHRAY_E_INVALID;
    if (!(c->cfg.flags & (BHRAY_F_TIMING | BHRAY_F_TIMING_SPARSE))) return fail(c, BHRAY_E_STATE, "ctx created without BHRAY_F_TIMING");
    int rc = dev_sync(c);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    const uint32_t nl = c->cfg.levels;
    uint64_t begin = c->timing_begin;
    if (c->batch_counter - begin > BHRAY_TIMING_RING) begin = c->batch_counter - BHRAY_TIMING_RING;
    for (uint64_t f = begin; f < c->batch_counter; f++) {
        const size_t ring = (size_t)(f % BHRAY_TIMING_RING);
        hipEvent_t* ev = batch_events(c, ring);
        if (!c->ring_frames[ring]) continue;                           // a batch without events (BHRAY_F_TIMING_SPARSE)
        if (c->sky_recorded[ring]) {
            float t = 0; HIPCHK(c, hipEventElapsedTime(&t, ev[ev_sky_begin(nl)], ev[ev_sky_end(nl)])); out->sky_ms += t; out->sky_launches++;
        }
        hipEvent_t first = nullptr, last = nullptr;
        for (uint32_t l = 0; l < nl; l++) {
            if (c->levels[l].rows.empty()) continue;
            float a = 0, b = 0;
            HIPCHK(c, hipEventElapsedTime(&a, ev[ev_level_begin(l)], ev[ev_level_classified(l)]));
            HIPCHK(c, hipEventElapsedTime(&b, ev[ev_level_classified(l)], ev[ev_level_traced(l)]));
            out->classify_ms += a; out->level_classify_ms[l] += a; out->classify_launches++;
            if (c->ring_own_trace[ring] >> l & 1) { out->trace_ms += b; out->level_trace_ms[l] += b; out->trace_launches++; }   // (the speculative and superset modes classify some levels only)
            if (!first) first = ev[ev_level_begin(l)];
            last = ev[ev_level_traced(l)];
        }
        if ((c->cfg.flags & BHRAY_F_TEMPORAL) && first) {      // prediction + predicted trace launch: the bulk of a temporal-mode frame
            float t = 0; HIPCHK(c, hipEventElapsedTime(&t, ev[ev_predicted_begin(nl)], ev[ev_predicted_end(nl)]));
            out->predicted_trace_ms += t; out->predicted_launches++;
            first = ev[ev_predicted_begin(nl)];
        }
        if (first && last) { float t = 0; HIPCHK(c, hipEventElapsedTime(&t, first, last)); out->total_ms += t; }
        out->frames += c->ring_frames[ring];
        out->batches++;
    }
    if (c->d_span) {
        std::vector<unsigned long long> sp((size_t)BHRAY_TIMING_RING * SPAN_MAX * 2);
        HIPCHK(c, hipMemcpy(sp.data(), c->d_span, sp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint64_t f = begin; f < c->batch_counter; f++) {
            const size_t ring = (size_t)(f % BHRAY_TIMING_RING);
            if (!c->ring_frames[ring]) continue;
            for (int t = 0; t < (int)c->ring_spans[ring]; t++) {
                const unsigned long long a = ~sp[(ring * SPAN_MAX + (size_t)t) * 2], b = sp[(ring * SPAN_MAX + (size_t)t) * 2 + 1];
                if (sp[(ring * SPAN_MAX + (size_t)t) * 2] == 0ull || b < a) continue;       // the launch never ran (no rows)
                out->trace_exec_ms += (float)((double)(b - a) / c->wall_clock_khz);
                out->trace_exec_launches++;
            }
        }
    }
    c->timing_begin = c->batch_counter;
    return BHRAY_OK;
}
