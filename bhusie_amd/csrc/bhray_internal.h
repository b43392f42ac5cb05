// bhray_internal.h — structures passed from the C-ABI host layer to the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bhray.h"

namespace bhray {

struct TexDev {
    const uint8_t* rgba;   // RGBA8 unorm, row-major, tightly packed (texture.rs:16-69)
    int w, h;
};

// Compact model resident in HBM.  Nodes are 32 B (two float4 halves); the two children of an
// inner node are adjacent (triangle.rs:239-243), so a child pair is one 64 B aligned read.
struct ModelDev {
    float pos[3];
    int visible;
    const float4* points;
    const float4* normals;
    const int32_t* triangles;   // 6 ints each
    const float4* nodes;        // 2 float4 per node
    const int32_t* lookup;
    const float4* leaf;         // pre-gathered leaf geometry: 6 float4 (p1,p2,p3,n1,n2,n3) per bvh_lookup slot
    int node_count;
    int root_cull;              // 1: root_lo/root_hi hold the union of the root's two child boxes (root is an inner node)
    float root_lo[3], root_hi[3];
};

// Everything that is uniform over a frame.  Lives in HBM (one entry per frame of a batch); the address is wave-uniform,
// so the members are fetched with scalar loads into SGPRs.
// Derived members are computed on the host with the SAME binary32 operation sequence the shader
// performs per pixel (ray.wgsl:270-281, 488, 511), so hoisting them cannot change a bit.
struct FrameParams {
    // camera (ray.wgsl:41-45, 269-285)
    float cam[3];
    float right[3];        // normalize(cross(forward, (0,-1,0)))
    float up[3];           // normalize(cross(forward, right))
    float fwd_ff[3];       // forward * (1 / tan(fov/2))
    float ray_distance;    // distance(camera.position, black_hole.position)  (ray.wgsl:511,555)
    float ray_distance_f;  // the same with the integrator's fused dot (N7): `dist` of a ray's first step
    int relativity0;       // ray_distance < relativity_radius                (ray.wgsl:488)
    // black hole (ray.wgsl:112-123)
    float bh[3];
    float bn[3];
    float bn_len;          // length(normal) (host), for the conservative disk cull
    float cull_outer_pad, cull_plane_c1, cull_plane_c2;   // black_hole_culls' folded constants: outer + 0.0501, 1.0101 |n|, 1.01e-4 |n|
    float inner, outer, rot_speed, R;
    int show_tex, show_shift;
    float M[9];            // rotation matrix columns c0,c1,c2
    float feather;
    // details (ray.wgsl:25-34)
    float time;
    float time_rot;        // time * rotation_speed (ray.wgsl:633): the same single binary32 product, formed once on the host
    int method;
    float step_size;
    int max_iter;
    float thr;
    float acos_cstar;      // largest c with bh_acos(c) >= thr (host, binary search): bh_acos(c) < thr <=> c > acos_cstar on [-1, 1]
    float acos_cstar_near; // the same for thr * temporal_margin (<= thr): temporal speculation also predicts the pixels this close to being traced
    int model_count;
    TexDev temp, disk, sky;
    ModelDev models[BHRAY_MAX_MODELS];
};

// One ladder level (one RayPipeline of the reference, ray_pipeline.rs:36-309).
struct LevelParams {
    int w, h;              // level size (textureDimensions(color_buffer))
    int pw, ph;            // previous level size; 1x1 => base case (ray.wgsl:178)
    float rx, ry;          // size_ratio (ray.wgsl:187), computed on the host in binary32
    const float4* prev;    // previous level, full pw*ph
    float4* out;           // this level's pixels
    int out_pitch;         // pixels per output row
    int out_x0;            // output column = x - out_x0
    const int32_t* rowmap; // level row y -> output row (nullptr: identity)
    const int32_t* rows;   // rows to compute (sorted), nrows entries
    int nrows;
    int x0, x1;            // columns to compute
    int tag;               // speculative mode: level id stored in bits 30-31 of the queue entries
    const float4* spec;    // speculative mode: already traced pixels of this level; a pixel that needs tracing copies from here
    int pass;              // CLASSIFY_NORMAL / CLASSIFY_TENTATIVE / CLASSIFY_KEEP (superset speculation, bhray_config.superset_levels)
    int no_store;          // tentative pass of the last level: nobody reads its image, only the queue entries are produced
};
enum : int { CLASSIFY_NORMAL = 0,
             // the coarser level may hold PENDING pixels (alpha = 2: queued for tracing, value not known yet).  A pixel whose inputs are all
             // known is classified exactly (copy / interpolate -> stored; trace -> queued, PENDING stored); a pixel with a PENDING
             // input is queued conservatively (a copy pixel: just marked PENDING).  The queued set is a superset of the exact one.
             CLASSIFY_TENTATIVE = 1,
             // after the trace of the superset: the coarser level is final.  Copy / interpolate are stored (overwriting speculative
             // traces the exact classification does not want); a pixel that needs tracing is left as the trace launch wrote it.
             CLASSIFY_KEEP = 2,
             // temporal speculation: exact classification (the coarser level is final).  Copy / interpolate are stored; a pixel that
             // needs tracing is recorded for the next frame's prediction and, unless this frame's predicted launch already traced it
             // (stamp), queued for this level's own trace launch.
             CLASSIFY_FIXUP = 3 };
#define BHRAY_PENDING_ALPHA 2.0f   // alpha of a final pixel is exactly 0 or 1

// Speculative tracing of several levels in one launch: per-level geometry and destination, selected by the entry's tag.
struct SpecLevel { int w, h; float4* out; int out_pitch; int out_x0; const int32_t* rowmap;    // rowmap/out_x0 as in LevelParams
                   uint32_t* stamp;      // temporal speculation: stamp[y*w + x] = FrameLaunch::stamp_value when the pixel is stored
                   unsigned long long* row_work; };   // counting builds: as FrameLaunch::row_work, for this level
struct SpecLevels { int n; SpecLevel l[BHRAY_MAX_SPEC_LEVELS]; };   // n == 0: one level, described by LevelParams

struct Counters64 { unsigned long long v[16]; };   // [0..12]: order = bhray_counters; [13..15]: the RK error-estimate bound (bhray_get_err_skip: wave-steps, all lanes pass, violations)

// One frame's share of one launch.  A launch covers the `nb` frames of a batch: classify uses blockIdx.y as the frame
// index, the persistent trace blocks start on frame blockIdx.x % nb and move on to the other frames when theirs runs dry.
struct FrameLaunch {
    LevelParams L;
    SpecLevels SL;
    uint32_t* queue;       // ray queue of this frame and level(s)
    uint32_t* qctl;        // [0] entries appended (classify), [1] entries taken (trace)
    Counters64* counters;  // nullptr unless BHRAY_F_COUNTERS
    unsigned long long* row_work;   // counting builds: row_work[y] += iterations of every ray traced for level row y (bhray_get_row_work); nullptr: off
    // temporal speculation (BHRAY_F_TEMPORAL): the exact classification records every pixel that needs tracing for the NEXT frame's
    // predicted launch, and sends to this frame's queue only those the predicted launch has not traced already
    uint8_t* need;         // this level's per-pixel mark "the shader traces this pixel" (written by the exact classification, read by predict_kernel)
    int radius;            // predict_kernel: dilation of the previous frame's traced set, in pixels of this level
    const uint32_t* stamp; // this level's stamp image (classify); nullptr outside temporal mode
    uint32_t stamp_value;  // stamp of the current frame
    int trace_flags;       // trace: TRACE_* bits below (scheduling only: no pixel depends on them)
    int blocks;            // predict (one launch, all levels): this level's own block count
    unsigned long long* span; // trace, entry 0 of a timed launch: [0] max(~first block start) [1] max(last block end), device wall clock; nullptr: untimed
    unsigned long long* work; // trace, entry 0 of a launch: work[blockIdx & (BHRAY_WORK_WORDS - 1)] += integrator steps this wave ISSUED for the frames of the batch
                              // (a step costs the wave the same whether 1 or 64 of its lanes march): what the batch's rays cost this GPU, whatever else shares
                              // it - the measure bhray_rebalance balances.  Counted in whole batches of BHRAY_REL_BATCH steps.
    uint32_t* qlen;           // trace: *qlen = qctl[0], the rays this frame's queue held for this launch, in pinned host memory: what the host sizes the NEXT launch of this
                              // slot position and ladder launch from (bhray_trace_grid_for; launch_batch).  One plain store by block 0; nullptr: not reported
};
// FrameLaunch::trace_flags
enum : int { TRACE_PROBE_EMPTY = 1,        // this launch is expected to find its queue (nearly) used up - look before the first atomic
             TRACE_THIN_STRIDED = 2,       // thin shares are dealt strided (a whole frame, one frame per launch)
             TRACE_QUAD_WPS_SHIFT = 2, TRACE_QUAD_WPS_MASK = 7,   // (flags >> shift) & mask: waves per SIMD the quad march may use (bhray_quad.inc); 0 = never
             TRACE_WAVE_PRIO = 32 };       // waves set their issue priority by their rays' predicted length
#define BHRAY_WORK_WORDS 16      // counters per frame (the waves of a launch spread over them: one word would serialise 2 048 atomics at every launch's end)
#define BHRAY_QCTL_WORDS (2 * BHRAY_MAX_LEVELS + 2 * BHRAY_WORK_WORDS)   // 32-bit words of a frame's control block: queue counts / heads, then the work counters (64-bit)

// classify / predict: a 256-thread block covers a rectangle of BX x BY 8x8-pixel tiles (4 waves, BX*BY/4 tiles each in turn)
#ifndef BHRAY_CLASSIFY_BX
#define BHRAY_CLASSIFY_BX 4
#endif
#ifndef BHRAY_CLASSIFY_BY
#define BHRAY_CLASSIFY_BY 2    // measured at 1080p RK, 20 slots: 4x1 5 315, 2x2 5 290, 4x2 5 406, 2x4 5 380, 4x4 5 360, 8x1 5 328, 8x2 5 345 Mrays/s
#endif
// launchers (bhray_kernels.hip); Pb / Fb are device arrays of nb entries
hipError_t launch_classify(const FrameParams* Pb, const FrameLaunch* Fb, int nb, int blocks, bool count, bool fixup, hipStream_t s);
// The build of trace_kernel a launch asks for.  models: 0 no usable visible model (the no-mesh kernels), 1 models tested in flat space only (the shader's behaviour), 2 also on
// every step inside the relativity sphere (bhray_set_mesh_lensing: the lensed-mesh kernels); dense: the build for a saturated device (no: the latency build);
// eval: 0 the numerics contract, 1 BHRAY_F_LITERAL, 2 BHRAY_F_EVAL_FMA; origin: every frame of the batch has the hole at +0, +0, +0;
// rays: the launch traces a caller's ray list, not a queue of pixels (bhray_trace_rays, DESIGN.md §15: trace_kernel's RAYS) - entry i of the launch IS ray i,
// FrameLaunch::L.prev holds the n records (bhray_ray: two float4 each), L.out the n results, qctl[0] = n; nothing else of L / SL / queue is read.
// records (implies rays): the launch also writes a bhray_ray_record per ray (bhray_trace_rays_records, DESIGN.md §16: trace_kernel's RECORDS) to the array FrameLaunch::row_work
// points at - the member only a counting launch reads, which a ray-list launch never is.
// paths (implies records): the launch also writes the sampled path of every ray (bhray_trace_rays_paths, DESIGN.md §17: trace_kernel's PATHS) - the points to the array
// FrameLaunch::need points at, the counts to FrameLaunch::stamp, with stride_log2 in FrameLaunch::radius and max_points in FrameLaunch::stamp_value: members of the
// classification and of temporal speculation, which a ray-list launch never reads.
struct TraceVariant { int method; int models; bool count; bool dense; int eval; bool origin; bool rays = false; bool records = false; bool paths = false; };
constexpr bool operator==(const TraceVariant& a, const TraceVariant& b) {
    return a.method == b.method && a.models == b.models && a.count == b.count && a.dense == b.dense && a.eval == b.eval && a.origin == b.origin && a.rays == b.rays && a.records == b.records && a.paths == b.paths;
}
#ifndef BHRAY_UNIFIED
#define BHRAY_UNIFIED 1          // (both described in bhray_kernels.hip; the defaults are needed here for trace_resolve, which is inline: EVERY translation unit that includes this
#endif                           // header must be built with the same -D as bhray_kernels.hip - the Makefile's EXTRA reaches the .hip rule, and only .hip files include it)
#ifndef BHRAY_ORIGIN_KERNEL
#define BHRAY_ORIGIN_KERNEL 1
#endif
// The build that runs when `asked` is asked for - the only place that knows the fallbacks.  Every build of a variant computes the same pixels, bit for bit, so a
// fallback costs time only.  What is instantiated is exactly the set of variants that resolve to themselves (bhray_kernels.hip: trace_kernel_ptr).
constexpr TraceVariant trace_resolve(TraceVariant v) {
    // ray lists: the contract's evaluation only (the API refuses the others), latency build, general hole position, no counting; models in flat space (1) or lensed (2:
    // bhray_set_mesh_lensing's BHRAY_LENS_RAYS) for ray lists and records - a path request folds to flat-space models (the API refuses paths under lensing)
    if (v.paths) v.records = true;                                            // the path kernels are record kernels
    if (v.records) v.rays = true;                                             // the record kernels are ray-list kernels
    if (v.rays) { if (v.paths && v.models == 2) v.models = 1; v.count = false; v.dense = false; v.eval = 0; v.origin = false; return v; }
    if (v.models == 2 && v.eval == 0) { v.dense = false; v.origin = false; return v; }   // lensed meshes: the latency general build, counting or not
    if (v.models == 2) v.models = 1;                                          // no lensed kernel under another evaluation (refused at bhray_set_mesh_lensing): flat-space models
    if (v.count || (v.eval != 0 && v.models != 0)) v.dense = false;           // dense builds exist where throughput is reported (trace_variant_exists, bhray_kernels.hip)
    if (!(BHRAY_ORIGIN_KERNEL != 0 && BHRAY_UNIFIED != 0 && v.eval == 0 && v.models == 0 && !v.count)) v.origin = false;   // ORIGIN builds: the no-mesh, non-counting contract kernels
    return v;
}
// (method, models, count, dense, eval, origin)
static_assert(trace_resolve({1, 0, true,  true,  0, false}) == TraceVariant{1, 0, true,  false, 0, false}, "trace_resolve");   // a dense counting request: latency
static_assert(trace_resolve({1, 1, false, true,  1, false}) == TraceVariant{1, 1, false, false, 1, false}, "trace_resolve");   // a dense mesh request under the literal / fma evaluations: latency
static_assert(trace_resolve({0, 1, false, true,  2, false}) == TraceVariant{0, 1, false, false, 2, false}, "trace_resolve");
static_assert(trace_resolve({1, 1, false, true,  0, false}) == TraceVariant{1, 1, false, true,  0, false}, "trace_resolve");   // ... under the contract: dense
static_assert(trace_resolve({1, 2, false, true,  0, true }) == TraceVariant{1, 2, false, false, 0, false}, "trace_resolve");   // lensed with dense and origin: latency and general, still lensed
static_assert(trace_resolve({0, 2, true,  true,  0, true }) == TraceVariant{0, 2, true,  false, 0, false}, "trace_resolve");
static_assert(trace_resolve({1, 2, false, false, 1, false}) == TraceVariant{1, 1, false, false, 1, false}, "trace_resolve");   // lensed under another evaluation: flat-space models
static_assert(trace_resolve({1, 0, false, true,  0, true }) == TraceVariant{1, 0, false, true,  0, BHRAY_ORIGIN_KERNEL != 0 && BHRAY_UNIFIED != 0}, "trace_resolve");   // origin survives for (contract, no mesh, no count), dense ...
static_assert(trace_resolve({0, 0, false, false, 0, true }) == TraceVariant{0, 0, false, false, 0, BHRAY_ORIGIN_KERNEL != 0 && BHRAY_UNIFIED != 0}, "trace_resolve");   // ... and latency, where the ORIGIN builds are built at all
static_assert(trace_resolve({1, 1, false, true,  0, true }) == TraceVariant{1, 1, false, true,  0, false}, "trace_resolve");   // origin is dropped for mesh,
static_assert(trace_resolve({1, 0, true,  false, 0, true }) == TraceVariant{1, 0, true,  false, 0, false}, "trace_resolve");   // for count
static_assert(trace_resolve({1, 0, false, true,  1, true }) == TraceVariant{1, 0, false, true,  1, false}, "trace_resolve");   // and for another evaluation
static_assert(trace_resolve({1, 0, false, true,  2, false}) == TraceVariant{1, 0, false, true,  2, false}, "trace_resolve");   // an already-resolved variant resolves to itself
static_assert(trace_resolve({1, 0, true,  true,  0, true,  true}) == TraceVariant{1, 0, false, false, 0, false, true}, "trace_resolve");   // a ray list: latency, general, not counting
static_assert(trace_resolve({0, 2, false, true,  0, false, true}) == TraceVariant{0, 2, false, false, 0, false, true}, "trace_resolve");   // ... and lensed models stay lensed
static_assert(!(trace_resolve({1, 0, false, false, 0, false, true}) == trace_resolve({1, 0, false, false, 0, false, false})), "trace_resolve: the ray-list kernels are builds of their own");
static_assert(trace_resolve({1, 2, true,  true,  0, true,  false, true}) == TraceVariant{1, 2, false, false, 0, false, true, true}, "trace_resolve");   // records imply a ray list, and resolve as one: lensed models stay lensed
static_assert(trace_resolve({1, 1, true,  true,  0, true,  false, true}) == TraceVariant{1, 1, false, false, 0, false, true, true}, "trace_resolve");   // ... flat-space models flat
static_assert(trace_resolve({0, 2, false, false, 0, false, true, true, false}) == TraceVariant{0, 2, false, false, 0, false, true, true, false}, "trace_resolve: the lensed record kernels are builds of their own");
static_assert(!(trace_resolve({1, 2, false, false, 0, false, true}) == trace_resolve({1, 1, false, false, 0, false, true})), "trace_resolve: the lensed ray-list kernels are builds of their own");
static_assert(trace_resolve({1, 2, false, false, 2, false, true}) == TraceVariant{1, 2, false, false, 0, false, true}, "trace_resolve");   // (a ray list's evaluation is the contract's: the API refuses the others before a launch)
static_assert(trace_resolve({0, 2, false, false, 0, false, true, true, true}) == TraceVariant{0, 1, false, false, 0, false, true, true, true}, "trace_resolve: no lensed path kernel - a path request folds to flat-space models");
static_assert(!(trace_resolve({0, 0, false, false, 0, false, true, true}) == trace_resolve({0, 0, false, false, 0, false, true, false})), "trace_resolve: the record kernels are builds of their own");
static_assert(trace_resolve({0, 1, false, false, 0, false, true, false}) == TraceVariant{0, 1, false, false, 0, false, true, false}, "trace_resolve");   // a ray list without records stays what it was
static_assert(trace_resolve({1, 2, true,  true,  0, true,  false, false, true}) == TraceVariant{1, 1, false, false, 0, false, true, true, true}, "trace_resolve");   // paths imply records, and resolve as a ray list
static_assert(!(trace_resolve({0, 0, false, false, 0, false, true, true, true}) == trace_resolve({0, 0, false, false, 0, false, true, true, false})), "trace_resolve: the path kernels are builds of their own");
static_assert(trace_resolve({0, 1, false, false, 0, false, true, true, false}) == TraceVariant{0, 1, false, false, 0, false, true, true, false}, "trace_resolve");   // a records request without paths stays what it was
static_assert(trace_resolve(trace_resolve(TraceVariant{0, 2, true, true, 2, true})) == trace_resolve(TraceVariant{0, 2, true, true, 2, true}), "trace_resolve is idempotent");
// launch_trace and trace_blocks_per_cu resolve `asked` themselves
hipError_t launch_trace(const FrameParams* Pb, const FrameLaunch* Fb, int nb, TraceVariant asked, int* err_flag, int grid_blocks, hipStream_t s);
int trace_blocks_per_cu(TraceVariant asked);
// copies n16 16-byte words from pinned host memory to device memory with a kernel (stays on the compute queue: a DMA copy
// between the launches of a stream costs a cross-engine handshake each time)
// and zeroes `nzero` 32-bit words at `zero` (the queue control words of the batch) in the same launch
hipError_t launch_upload(const void* pinned_src, void* dst, size_t n16, uint32_t* zero, size_t nzero, hipStream_t s);
hipError_t launch_predict(const FrameParams* Pb, const FrameLaunch* Fb, int nb, int levels, int blocks, hipStream_t s);   // temporal speculation: F.need -> F.queue
hipError_t launch_selftest(unsigned long long* bad3, hipStream_t s);   // [0]: 1/x mismatches, [1]: sqrt mismatches, [2]: places where bh_acos increases
hipError_t launch_sky(const TexDev& sky, const float4* src, uint2* dst_rgba16f, size_t npix, hipStream_t s);

// display pass (bhray_post.hip): bloom down x5 / up x5, mix, ACES, FXAA into RGBA8 sRGB
#define BHRAY_BLOOM_LEVELS 10
struct PostArgs {                        // fxaa_kernel's arguments: the uniform block, and the sRGB encoding's decision thresholds (copied to LDS)
    float srgb_thr[255];                 // increasing: byte = number of thresholds <= the value
    float edge_min, edge_max;
    int iterations;
    float subpix;
    float one_twelfth;                   // fxaa.wgsl's `1.0 / 12.0` (an abstract-float constant, rounded to f32 once)
};
int bloom_sizes(uint32_t frame_w, uint32_t frame_h, uint32_t w[BHRAY_BLOOM_LEVELS], uint32_t h[BHRAY_BLOOM_LEVELS]);   // BHRAY_E_INVALID: a level would be empty
size_t display_scratch_bytes(uint32_t frame_w, uint32_t frame_h);                  // device bytes launch_display needs besides its input and output; 0: frame too small
// the 11 launches of the display pass on stream s: RGBA16F sky image (frame_w x frame_h) -> RGBA8 sRGB image
hipError_t launch_display(const uint2* sky, uint2* scratch, uint32_t* dst_rgba8, uint32_t frame_w, uint32_t frame_h,
                          const bhray_fxaa_details& fxaa, const bhray_mix_details& mix, hipStream_t s);
// launch_display's last launch alone: fxaa_kernel over a tone-mapped RGBA16F image (bhray_diag_display_image's BHRAY_DIAG_DISPLAY_FXAA_ONLY)
hipError_t launch_fxaa(const uint2* tone, uint32_t* dst_rgba8, uint32_t frame_w, uint32_t frame_h, const bhray_fxaa_details& fxaa, hipStream_t s);

// mesh BVH built on the device (bhray_bvh.hip)
struct BvhBuild;                         // scratch of one model slot's builder: allocated once per upload, reused by every vertex update
struct BvhResult {                       // what a build reports: 64 bytes read back behind it
    uint32_t nodes, leaves, max_leaf, max_depth;   // max_depth: nodes on the longest path root -> leaf; 0 = the fit passes did not reach the root
    int32_t root_cull;                   // as ModelDev
    float root_lo[3], root_hi[3];
    uint32_t pad[5];
};
static_assert(sizeof(BvhResult) == 64, "BvhResult");
hipError_t bvh_build_create(int triangle_count, BvhBuild** out);          // triangle_count >= 1
void bvh_build_destroy(BvhBuild* b);
// every p* < point_count and n* < normal_count (and >= 0)?  *host_error != 0: no.  Synchronises s.
hipError_t launch_bvh_validate(BvhBuild* b, const int32_t* triangles, int point_count, int normal_count, int* host_error, hipStream_t s);
// nodes: room for 2 T - 1 nodes; lookup: T; leaf: 6 T float4.  Enqueues only.
hipError_t launch_bvh_build(BvhBuild* b, const float4* points, const float4* normals, const int32_t* triangles, float4* nodes, int32_t* lookup, float4* leaf,
                            BvhResult* d_result, hipStream_t s);
// The affine pose of DESIGN.md §14: points[i] = A rest_points[i] + t, normals[i] = A rest_normals[i] (w copied), pose = row-major 3x4 (A | t).  One launch over
// point_count + normal_count vertices; the counts are independent and either may be 0.  Enqueues only.
hipError_t launch_bvh_pose(const float4* rest_points, const float4* rest_normals, float4* points, float4* normals, int point_count, int normal_count,
                           const float pose[12], hipStream_t s);

}  // namespace bhray
