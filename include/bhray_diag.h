/*
 * bhray_diag.h — measurement and verification entry points of libbhray.
 *
 * bhray.h is what a renderer calls (a RayPipeline shim; the C++ host, host/renderer.hpp).  This header
 * adds what exists to MEASURE or VERIFY the library rather than to render a frame: the counters and the row work of the
 * counting build, the HIP-event timing, the device self-test, the read-back of any ladder level, the display pass over a supplied image and the gather statistics.
 * The tests, bench.py and the profiling scripts use them; a product host needs none.  It includes bhray.h, so a diagnostic
 * consumer includes this file only.  The conventions of bhray.h hold here too.
 */
#ifndef BHRAY_DIAG_H
#define BHRAY_DIAG_H

#include "bhray.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Measurement flags of bhray_config.flags (the values are bhray.h's BHRAY_F_* enum)
 *
 * BHRAY_F_COUNTERS       kernels also accumulate bhray_counters (slower).
 * BHRAY_F_TIMING         record HIP events around every launch.
 * BHRAY_F_TIMING_SPARSE  like BHRAY_F_TIMING, but only every 4th batch carries events (a recorded event is a packet in
 *                        the stream: 12 per frame cost a saturated device 1.6 %); bhray_get_timing aggregates those.
 * BHRAY_F_LITERAL        the integrator (ray.wgsl:401-480, 533) operator by operator: one binary32 operation per
 *                        WGSL operator in source order, no fused multiply-add, no reassociation.  Slower; exists
 *                        to MEASURE how far the default evaluation (DESIGN.md §2, N3/N7/N9/N10 — permitted by
 *                        WGSL, cheaper on CDNA4) is from the shader text: tests/test_gpu_literal.py.  Cost: bench.py's
 *                        `literal` entry.
 * BHRAY_F_EVAL_FMA       a THIRD evaluation of the integrator: the shader text with fused multiply-add contraction only
 *                        (every `x*y + z` of ray.wgsl:401-480 one fma), none of the contract's reassociations (N9/N10).
 *                        Like BHRAY_F_LITERAL it exists for measurement: the pixels on which it differs from the literal
 *                        text by more than 1e-4 are the pixels on which the default evaluation does
 *                        (tests/test_gpu_literal.py).  Ignored when BHRAY_F_LITERAL is set.
 * ---------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------
 * Counters (BHRAY_F_COUNTERS)
 * ---------------------------------------------------------------------------------------- */
typedef struct bhray_counters {        /* summed over all levels of the last render          */
    uint64_t pixels;                   /* pixels written (all levels)                        */
    uint64_t copied;                   /* grid: copied from the coarser level (ray.wgsl:193) */
    uint64_t interpolated;             /* grid: bilinear mix of directions (ray.wgsl:217)    */
    uint64_t traced;                   /* pixels that ran trace_ray                          */
    uint64_t steps;                    /* relativity iterations (integrator steps)           */
    uint64_t flat_iters;               /* flat-space iterations                              */
    uint64_t node_pairs;               /* BVH inner-node visits (2 AABB tests each)          */
    uint64_t triangles;                /* hit_triangle calls                                 */
    uint64_t disk_hits;                /* accretion-disk shading events                      */
    uint64_t sky_samples;              /* in-kernel sky taps (ray.wgsl:587)                  */
    /* scheduling of the trace kernel (not a property of the frame: depends on frames in flight, batches, the kernel build)   */
    uint64_t wave_steps;               /* integrator steps issued by waves: `steps` / (64 * wave_steps) = fraction of the lanes
                                          of a stepping wave that hold a live ray                                            */
    uint64_t rays_adopted;             /* rays that changed wave through the drain-merging mailbox (dense build)             */
    uint64_t max_ray_iterations;       /* iterations of the longest ray (a maximum, also over levels): the latency floor of a level
                                          is its longest ray                                                                  */
} bhray_counters;
int bhray_get_counters(bhray_ctx* ctx, bhray_counters* out);   /* needs BHRAY_F_COUNTERS     */
int bhray_get_level_counters(bhray_ctx* ctx, uint32_t level, bhray_counters* out);
/* Where the work of the last render lies: out[y] = iterations of all rays traced for row y of ladder level `level` (n = level_h[level]
 * numbers; rows this ctx did not render are 0; a multi-partition ctx sums its local partitions).  Needs BHRAY_F_COUNTERS.
 * The input of bhray_balance_slabs.                                                                                              */
int bhray_get_row_work(bhray_ctx* ctx, uint32_t level, uint64_t* out, uint32_t n);

/* ------------------------------------------------------------------------------------------
 * Timing (BHRAY_F_TIMING, BHRAY_F_TIMING_SPARSE)
 * ---------------------------------------------------------------------------------------- */
/* HIP-event timing of every launch (events recorded on the ctx stream).  bhray_get_timing sums
 * over the batches launched since the previous call (at most BHRAY_TIMING_RING of them).     */
#define BHRAY_TIMING_RING 128
typedef struct bhray_timing {
    uint32_t frames;                   /* frames aggregated                                  */
    uint32_t batches;                  /* batches aggregated (= frames unless frames_per_batch > 1) */
    float    total_ms;                 /* Σ (first launch → last launch) per batch           */
    float    trace_ms;                 /* Σ trace kernels                                    */
    float    classify_ms;              /* Σ grid classify kernels                            */
    uint32_t trace_launches;
    uint32_t classify_launches;
    float    level_trace_ms[BHRAY_MAX_LEVELS];
    float    level_classify_ms[BHRAY_MAX_LEVELS];
    float    sky_ms;                   /* Σ sky resolve kernels                              */
    uint32_t sky_launches;
    float    gather_ms;                /* multi-GPU, root: Σ (receive of the row tiles: start → all tiles arrived)   */
    float    deinterleave_ms;          /* multi-GPU, root: Σ de-interleave kernels                                   */
    uint32_t gathers;                  /* batches gathered                                                            */
    float    predicted_trace_ms;       /* BHRAY_F_TEMPORAL: Σ (prediction + the predicted trace launch, all levels): the bulk of such a
                                          frame; trace_ms / level_trace_ms then hold the fix-up launches only          */
    uint32_t predicted_launches;
    float    trace_exec_ms;            /* Σ EXECUTION spans of the trace kernels: first block's start → last block's end on the device's
                                          constant-rate clock, stamped by the kernel itself.  trace_ms (HIP events in the stream) also
                                          contains the time a launch waits for room beside the persistent kernels of the other frames
                                          in flight; this is what `rocprofv3 --kernel-trace` reports as the kernel's duration          */
    uint32_t trace_exec_launches;
} bhray_timing;
int bhray_get_timing(bhray_ctx* ctx, bhray_timing* out);       /* needs BHRAY_F_TIMING       */

/* ------------------------------------------------------------------------------------------
 * Verification
 * ---------------------------------------------------------------------------------------- */
/* Device self-test of the properties two exact shortcuts rest on: (i) the integrator computes the correctly
 * rounded 1/x and sqrt(x) with short gfx950 sequences — run against the IEEE lowering on all 2^32 binary32 bit patterns;
 * (ii) the grid classification replaces `acos(c) < threshold` by `c > c*` — the portable acos must be monotone over every
 * binary32 value of [-1, 1].  Returns the number of violating inputs of each (all must be 0).  ~20 ms.              */
int bhray_selftest(bhray_ctx* ctx, uint64_t mismatches[3]);    /* [0] = 1/x and the step-size power, [1] = sqrt, [2] = acos monotonicity */

/* Which build of the trace kernels the launches got: launches[0] = trace launches enqueued since create with an ORIGIN build (the hole at
 * +0, +0, +0 in every frame of the batch: the march without position - hole), launches[1] = with any other build; summed over the local
 * partitions.  Frames staged but not yet launched (frames_per_batch > 1) are not counted: bhray_flush or bhray_sync first.  The pixels do
 * not depend on the build; BHRAY_ORIGIN_KERNEL=0 in the environment at create: never an ORIGIN build.                      */
int bhray_get_trace_builds(bhray_ctx* ctx, uint64_t launches[2]);

/* Trace grids sized by queue length.  Every dense-build trace launch of the ladder - the speculative levels' merged launch, each plain level, the
 * superset launch - reports the rays its queues held to the host, and the next batch staged at the same slot sizes that launch's persistent grid from it:
 *   blocks = ceil(expected_rays * (100 + margin_percent) / 100 / rays_per_block_generation), clamped to [max(frames_in_batch, floor_blocks), ctx_grid].
 * expected_rays = BHRAY_LEVEL_GRID_NO_FEEDBACK (nothing reported yet: a new ctx, a new partition, another kernel variant): ctx_grid, the grid every launch had before.
 * The ceiling wins over the floor.  Scheduling only: persistent waves pull until the queues are exhausted, so a grid that is too small makes a launch longer and
 * changes no pixel.  Environment at create: BHRAY_LEVEL_GRID=0 off (every launch gets ctx_grid), BHRAY_LEVEL_GRID_GEN (256), BHRAY_LEVEL_GRID_MARGIN (25),
 * BHRAY_LEVEL_GRID_FLOOR (64).  Never sized: latency-build launches, the temporal mode's launches, counting ctxs.                                               */
#define BHRAY_LEVEL_GRID_NO_FEEDBACK UINT64_MAX
uint32_t bhray_trace_grid_for(uint64_t expected_rays, uint32_t frames_in_batch, uint32_t ctx_grid, uint32_t rays_per_block_generation,
                              uint32_t margin_percent, uint32_t floor_blocks);
/* What the rule did.  Launch ids: 0 the speculative levels' merged launch, 1 + l the plain launch of level l, BHRAY_MAX_LEVELS + 1 the superset launch. */
#define BHRAY_LEVEL_GRID_LAUNCHES (BHRAY_MAX_LEVELS + 2)
typedef struct bhray_level_grid_info {
    uint64_t expected_rays[BHRAY_LEVEL_GRID_LAUNCHES];  /* the batch `slot` launched last: what each trace launch was sized from (summed over the batch's frames);
                                                           BHRAY_LEVEL_GRID_NO_FEEDBACK: not sized (no feedback, the rule off, or a launch the rule leaves alone)   */
    uint64_t total_launches;           /* since create, local partitions summed: ladder trace launches enqueued ...                                                  */
    uint64_t total_blocks;             /* ... the blocks they had together ...                                                                                       */
    uint64_t total_ceiling_launches;   /* ... and how many of them kept their unsized grid                                                                              */
    uint32_t blocks[BHRAY_LEVEL_GRID_LAUNCHES];         /* blocks each trace launch of that batch got; 0: the batch had no such launch                               */
    uint32_t enabled;                  /* 1: this ctx sizes its dense ladder launches (not BHRAY_LEVEL_GRID=0, no counters, not temporal)                            */
    uint32_t frames;                   /* frames of that batch (0: the slot has launched nothing)                                                                    */
    uint32_t ctx_grid;                 /* the ceiling of that batch                                                                                                  */
    uint32_t dense;                    /* 1: the batch's trace launches RAN dense builds                                                                             */
} bhray_level_grid_info;
/* slot < frames_in_flight; per-batch fields from the first local partition.  Host state only: no synchronisation. */
int bhray_get_level_grids(bhray_ctx* ctx, uint32_t slot, bhray_level_grid_info* out);

/* The Cash-Karp step skips its error estimate where a bound on it - (dist + 1) * (s*h)^2 <= 3.6e-5, proved above next_ray_rk_t in bhray_kernels.hip - shows every active
 * lane of the wave below the step-size controller's threshold.  The counting kernels (BHRAY_F_COUNTERS) always form the estimate and count, for the RK
 * steps of the last render, summed over levels and local partitions: out[0] = wave-steps, out[1] = wave-steps whose active lanes all satisfied the bound (what a
 * skipping build skips), out[2] = lane-steps that satisfied the bound with an estimate ABOVE the threshold - the proof's claim measured on the device: must be 0.
 * All 0 for Euler, the literal / fma evaluations and a library built with -DBHRAY_ERR_SKIP=0.                                                                      */
int bhray_get_err_skip(bhray_ctx* ctx, uint64_t out[3]);       /* needs BHRAY_F_COUNTERS     */

/* Any ladder level, full size level_w×level_h (unrendered pixels are NaN-filled at create).  */
int bhray_read_level(bhray_ctx* ctx, uint32_t level, float* dst_rgba32f, size_t row_pitch_bytes);

/* ------------------------------------------------------------------------------------------
 * Device-built trees (bhray_upload_model_build)
 * ---------------------------------------------------------------------------------------- */
/* What the last build of a slot produced (first local partition).  A host-built slot: built_on_device 0, triangles and nodes
 * filled, the rest 0.  An empty slot: BHRAY_E_STATE.                                                                  */
typedef struct bhray_model_build_info {
    uint32_t built_on_device, triangles, nodes, leaves, max_leaf, max_depth;
    float    upload_ms, build_ms;   /* HIP events around the copies / the build kernels of the last build; after
                                       bhray_set_model_pose the pose kernel stands where the copies stood (upload_ms is its time) */
} bhray_model_build_info;
int bhray_get_model_build_info(bhray_ctx* ctx, uint32_t model_index, bhray_model_build_info* out);
/* The tree a slot holds on the device (any slot, host-built ones too; first local partition): node_count nodes in
 * the device's numbering and triangle_count lookup entries.  Caps too small: BHRAY_E_INVALID, counts still written. */
int bhray_read_model_bvh(bhray_ctx* ctx, uint32_t model_index, bhray_node* nodes, uint32_t node_cap, int32_t* lookup,
                         uint32_t lookup_cap, uint32_t* node_count, uint32_t* triangle_count);
/* The points / normals a slot's kernels read now (posed, if a pose is in force: DESIGN.md §14; first local partition), 4 floats
 * each.  Either pointer may be NULL (that array is not read).  Caps too small: BHRAY_E_INVALID, counts still written.
 * A slot of 0 triangles holds no arrays: both counts are 0.                                                            */
int bhray_read_model_vertices(bhray_ctx* ctx, uint32_t model_index, float* points, uint32_t point_cap, float* normals, uint32_t normal_cap,
                              uint32_t* point_count, uint32_t* normal_count);

/* ------------------------------------------------------------------------------------------
 * The accumulation image (bhray_accum_*)
 * ---------------------------------------------------------------------------------------- */
/* The records the generator kernel writes for sample s under the current uniforms and the still camera in force
 * (bhray_accum_set_camera): frame_w * frame_h of them, row 0 the top, x fastest.  With an observer in force
 * (bhray_accum_set_observer, a velocity other than zero) they are the boosted records the observer's generator writes;
 * without one they are unchanged.  Needs no bhray_accum_begin; s >= BHRAY_ACCUM_MAX_SAMPLES or a NULL out:
 * BHRAY_E_INVALID; the refused states of bhray_accum_add apart from mesh lensing (the generator does not trace).  Waits. */
int bhray_accum_sample_rays(bhray_ctx* ctx, uint32_t s, bhray_ray* out);
/* bhray_still_sample_rays_host (below) under an observer: the function the observer's kernels call,
 * compiled for the host - the boosted records into out_rays and each record's beam D^4 into out_beam (may be NULL).
 * observer NULL or of zero velocity: the still camera's records, beam 1.  Needs no ctx and no device.  BHRAY_E_INVALID:
 * what bhray_still_sample_rays_host refuses, or an observer that bhray_accum_set_observer refuses.                    */
int bhray_observer_sample_rays_host(const bhray_config* cfg, const void* camera_uniform_32, const bhray_still_camera* camera, const bhray_observer* observer, uint32_t s,
                                    bhray_ray* out_rays, float* out_beam);
/* The same records by host arithmetic: the function the still-camera kernels call, compiled for the
 * host, over the frame of `cfg`, the 32 bytes of a bhray_camera_uniform and `camera` (NULL: the default; then the
 * records are those of the pinhole generator).  Needs no ctx and no device.  BHRAY_E_INVALID: a NULL cfg, uniform or
 * out, s >= BHRAY_ACCUM_MAX_SAMPLES, a cfg that is no ladder with a frame inside its last level, a camera that
 * bhray_accum_set_camera refuses.                                                                                     */
int bhray_still_sample_rays_host(const bhray_config* cfg, const void* camera_uniform_32, const bhray_still_camera* camera, uint32_t s, bhray_ray* out);
/* At most max_rays rays per trace launch of bhray_accum_add: K = max(1, max_rays / (frame_w * frame_h)) samples go
 * into one launch.  0 restores the default, 2^22; more than BHRAY_MAX_RAYS_PER_CALL: BHRAY_E_INVALID.  The image
 * does not depend on it.                                                                                             */
int bhray_accum_set_launch_rays(bhray_ctx* ctx, uint32_t max_rays);
/* The launches of bhray_accum_read_denoised with a HIP event between them, no image delivered: ms[0] is the
 * prepare launch, ms[1 + i] the a-trous launch of iteration i (tap spacing 1 << i), 0 for the iterations p does not ask
 * for.  Milliseconds of device time.  Refuses what bhray_accum_read_denoised refuses; a NULL ms: BHRAY_E_INVALID.  Changes
 * no accumulation state.  Waits.                                                                                       */
int bhray_accum_denoise_times(bhray_ctx* ctx, const bhray_still_denoise* p, float ms[6]);
/* One selection of bhray_accum_add_adaptive under `params` without sampling: the frame pixels
 * (y * frame_w + x) with issued < max_samples that are not converged, in the order the selection kernel compacted them
 * (unspecified between blocks).  *n is their number, the first min(*n, cap) go to out (out may be NULL when cap is
 * 0).  params is checked as bhray_accum_add_adaptive checks it (min_samples / round_samples against the first adaptive
 * call's, if there was one); BHRAY_E_STATE before bhray_accum_begin and in a uniform accumulation.  Changes nothing.
 * Waits.                                                                                                             */
int bhray_accum_active_pixels(bhray_ctx* ctx, const bhray_accum_adaptive* params, uint32_t* out, uint32_t cap, uint32_t* n);

/* ------------------------------------------------------------------------------------------
 * The footprint-filtered sky pass (bhray_set_sky_filter)
 * ---------------------------------------------------------------------------------------- */
/* Level `level` >= 1 of the sky pyramid as the filter kernel reads it: lw x lh texels (bhray_sky_pyramid_sizes) of four binary16,
 * row 0 the top; `texels` must be lw * lh.  BHRAY_E_STATE while the mode is off or no sky texture is resident; BHRAY_E_INVALID for
 * level 0 (that is the texture), a level beyond the top, a NULL dst or another texel count.  Waits.                               */
int bhray_read_sky_pyramid_level(bhray_ctx* ctx, uint32_t level, uint16_t* dst_rgba16f, size_t texels);

/* ------------------------------------------------------------------------------------------
 * The display pass over a supplied image
 * ---------------------------------------------------------------------------------------- */
/* Runs the display pass a ctx runs behind its sky pass - the same launches - over a caller's image, so that the kernels can be
 * held to images no device rendered.  No ctx: device memory is allocated, the w x h RGBA16F image (four binary16 per pixel, row
 * 0 the top, tightly packed) copied in, the pass run and waited for, dst_rgba8 (w x h x 4 bytes) copied back, everything freed.
 * fxaa_16 / mix_4: the bytes of a bhray_fxaa_details / bhray_mix_details; NULL: what bhray_post_defaults gives.
 * stages_rgba16f, if not NULL, receives what the pass leaves in its scratch, in its order: bloom levels 0 to 8 (sizes from
 * bhray_bloom_sizes), then the tone-mapped w x h image; stage_texels must be exactly that many texels (ignored when the pointer
 * is NULL).  Level 9 and the mixed image are never in memory: the last kernel fuses them.
 * BHRAY_DIAG_DISPLAY_FXAA_ONLY: the image is taken as the tone-mapped one and the last launch (FXAA and the RGBA8 store) runs
 * alone; mix_4 is not read and stages_rgba16f must be NULL.
 * BHRAY_E_INVALID: a NULL image or dst, an unknown flag bit, a frame bhray_bloom_sizes refuses (with the flag too) or wider or
 * higher than 32767, iterations above BHRAY_FXAA_MAX_ITERATIONS, a stage buffer of another size or beside the flag - all
 * checked before the device is touched.  BHRAY_E_NO_DEVICE: no device, or `device` not among the visible ones.  The message
 * is bhray_last_error(NULL)'s.                                                                                                  */
#define BHRAY_DIAG_DISPLAY_FXAA_ONLY 1u
int bhray_diag_display_image(int device, const uint16_t* rgba16f, uint32_t w, uint32_t h, const void* fxaa_16, const void* mix_4, uint32_t flags,
                             uint8_t* dst_rgba8, uint16_t* stages_rgba16f, size_t stage_texels);

/* ------------------------------------------------------------------------------------------
 * Point stars over a supplied image (bhray_set_stars)
 * ---------------------------------------------------------------------------------------- */
/* Runs the star kernel a ctx runs behind its sky pass, with the ctx's catalogue and parameters, over a caller's frame - so that the
 * kernel can be held to frames the tracer would never produce (exact ties, frames smaller than a tile).  frame_rgba32f: w x h pixels
 * of four floats, row 0 the top, tightly packed, as bhray_read_hdr delivers them; sky_in_rgba16f: the w x h RGBA16F image the stars
 * are added to (NULL: zeros); sky_out_rgba16f receives the image.  Device memory is allocated, the pass run on the legacy stream and
 * waited for, everything freed; the ctx's frames are not touched.  BHRAY_E_STATE: the ctx has no catalogue (or is not a
 * single-device ctx).  BHRAY_E_INVALID: NULL frame or output, w or h == 0 or above 32767.                                        */
int bhray_diag_star_image(bhray_ctx* ctx, const float* frame_rgba32f, uint32_t w, uint32_t h, const uint16_t* sky_in_rgba16f, uint16_t* sky_out_rgba16f);
/* What rules 2 - 6 did at every pixel of a frame, on the host (bhray_stars_resolve_host's loop): what the cost measurement and the
 * tests' coverage floors count.  Arguments and errors as bhray_stars_resolve_host's.                                              */
typedef struct bhray_star_pixel_info {
    uint32_t state;                     /* 0 summed, 1 skipped by max_footprint, 2 skipped by BHRAY_STARS_MAX_CELLS, 3 no footprint */
    uint32_t faces, cells;              /* faces visited, cells in their boxes                                                   */
    uint32_t tested, accepted, reversed;/* stars the inside test ran on, stars accepted, those of them by the reversed-sign form   */
    float    area;                      /* A of rule 3 (before min_area)                                                         */
    uint32_t pad;
} bhray_star_pixel_info;                /* 32 B */
int bhray_diag_stars_pixel_info_host(const float* frame_rgba32f, uint32_t w, uint32_t h, const bhray_star* stars, uint32_t n,
                                     const bhray_star_params* params, bhray_star_pixel_info* info);

/* ------------------------------------------------------------------------------------------
 * Gather statistics (multi-GPU)
 * ---------------------------------------------------------------------------------------- */
/* What a ctx gathers with.                                                                                          */
typedef struct bhray_gather_info {
    uint32_t partitions;                /* row partitions of the frame (1 = no tiling)                               */
    uint32_t local_partitions;          /* partitions rendered by this ctx                                           */
    uint32_t root;                      /* partition that receives the frame                                         */
    uint32_t root_is_local;             /* 1: the frame is delivered by this ctx                                     */
    uint32_t comm_ranks;                /* ranks of the RCCL communicator (0: no gather)                             */
    uint32_t rccl_version;              /* ncclGetVersion, e.g. 22707 (0: RCCL not loaded)                           */
    uint64_t bytes_sent_per_frame;      /* by this ctx's non-root partitions                                         */
    uint64_t bytes_received_per_frame;  /* by the root partition (0 when it is not local)                            */
} bhray_gather_info;
int bhray_get_gather_info(const bhray_ctx* ctx, bhray_gather_info* out);

#ifdef __cplusplus
}
#endif
#endif /* BHRAY_DIAG_H */
