// bhray_layout.cpp — compile-time proof that include/bhray.h carries the reference's byte layouts.
//
// Every size and offset the Rust host's #[repr(C)] structs (and the WGSL structs they mirror) define is asserted here, so a
// drift of the header cannot compile.  Sources: RayDetails ray_pipeline.rs:3-14 (ray.wgsl:25-34); CameraUniform
// camera.rs:66-73 (ray.wgsl:41-45); BlackHoleUniform blackhole.rs:37-51 (ray.wgsl:112-123); NodeUniform triangle.rs:45-52
// (ray.wgsl:85-90); Triangle triangle.rs:54-63 (ray.wgsl:67-74); ModelUniform triangle.rs:268-285 (ray.wgsl:47-65);
// MaterialUniform material.rs:7-11.
#include <stddef.h>

#include "../../include/bhray_diag.h"   // bhray.h, and bhray_counters for the size below

#define OFF(T, m, v) static_assert(offsetof(T, m) == (v), #T "." #m " offset")
#define SZ(T, v) static_assert(sizeof(T) == (v), #T " size")

SZ(bhray_details, 32);
OFF(bhray_details, material_count, 0); OFF(bhray_details, model_count, 4); OFF(bhray_details, time, 8);
OFF(bhray_details, integration_method, 12); OFF(bhray_details, step_size, 16); OFF(bhray_details, max_iterations, 20);
OFF(bhray_details, angle_division_threshold, 24); OFF(bhray_details, highlight_interpolation, 28);

SZ(bhray_camera_uniform, 32);
OFF(bhray_camera_uniform, position, 0); OFF(bhray_camera_uniform, _padding, 12); OFF(bhray_camera_uniform, forward, 16);
OFF(bhray_camera_uniform, fov, 28);

SZ(bhray_black_hole_uniform, 132);
OFF(bhray_black_hole_uniform, accretion_disk_inner, 0); OFF(bhray_black_hole_uniform, accretion_disk_outer, 4);
OFF(bhray_black_hole_uniform, rotation_speed, 8); OFF(bhray_black_hole_uniform, relativity_sphere_radius, 12);
OFF(bhray_black_hole_uniform, position, 16); OFF(bhray_black_hole_uniform, show_disk_texture, 28);
OFF(bhray_black_hole_uniform, normal, 32); OFF(bhray_black_hole_uniform, show_red_shift, 44);
OFF(bhray_black_hole_uniform, rotation_matrix, 48); OFF(bhray_black_hole_uniform, feather_amount, 96);
OFF(bhray_black_hole_uniform, pad, 100);

SZ(bhray_node, 32);
OFF(bhray_node, min_corner, 0); OFF(bhray_node, left_child, 12); OFF(bhray_node, max_corner, 16); OFF(bhray_node, obj_count, 28);

SZ(bhray_triangle, 24);
OFF(bhray_triangle, p1, 0); OFF(bhray_triangle, p2, 4); OFF(bhray_triangle, p3, 8);
OFF(bhray_triangle, n1, 12); OFF(bhray_triangle, n2, 16); OFF(bhray_triangle, n3, 20);

// ModelUniform: 48-byte header, then points / normals (vec4 each), triangles (24 B), nodes (32 B), bvh_lookup (4 B),
// each BHRAY_MAX_MODEL_VERTICES long, then 28 bytes of tail padding (triangle.rs:268-285)
SZ(bhray_model_header, 48);
OFF(bhray_model_header, position, 0); OFF(bhray_model_header, visible, 12); OFF(bhray_model_header, rotation, 16);
OFF(bhray_model_header, pad3, 28); OFF(bhray_model_header, point_count, 32); OFF(bhray_model_header, normal_count, 36);
OFF(bhray_model_header, triangle_count, 40); OFF(bhray_model_header, pad0, 44);
static_assert(BHRAY_MAX_MODEL_VERTICES == 524288, "triangle.rs:7");
static_assert(BHRAY_MODEL_OFF_POINTS == 48u, "points");
static_assert(BHRAY_MODEL_OFF_NORMALS == 8388656u, "normals = 48 + 16 * 524288");
static_assert(BHRAY_MODEL_OFF_TRIANGLES == 16777264u, "triangles = normals + 16 * 524288");
static_assert(BHRAY_MODEL_OFF_NODES == 29360176u, "nodes = triangles + 24 * 524288");
static_assert(BHRAY_MODEL_OFF_LOOKUP == 46137392u, "bvh_lookup = nodes + 32 * 524288");
static_assert(BHRAY_MODEL_OFF_LOOKUP + 4u * BHRAY_MAX_MODEL_VERTICES + 28u == BHRAY_MODEL_UNIFORM_BYTES, "ModelUniform size");
static_assert(BHRAY_MODEL_UNIFORM_BYTES == 48234572u, "ModelUniform size (triangle.rs:268-285)");
static_assert(BHRAY_MAX_MODELS == 8 && BHRAY_MAX_MATERIALS == 8, "ray.wgsl:2 MAX_MODELS raised from 1 (bhray.h), material.rs:3");

// FXAADetailsUniform (fxaa_pipline.rs:76-83) and MixDetails (mix_pipeline.rs:5-7): the display pass's uniform blocks
SZ(bhray_fxaa_details, 16);
OFF(bhray_fxaa_details, edge_threshold_min, 0); OFF(bhray_fxaa_details, edge_threshold_max, 4); OFF(bhray_fxaa_details, iterations, 8);
OFF(bhray_fxaa_details, subpixel_quality, 12);
SZ(bhray_mix_details, 4);
OFF(bhray_mix_details, mix_ratio, 0);

// a ray of bhray_trace_rays: two 16-byte halves (the kernel loads it as two float4)
SZ(bhray_ray, 32);
OFF(bhray_ray, origin, 0); OFF(bhray_ray, pad0, 12); OFF(bhray_ray, direction, 16); OFF(bhray_ray, pad1, 28);
static_assert(BHRAY_MAX_RAYS_PER_CALL == (1u << 26), "BHRAY_MAX_RAYS_PER_CALL");
// a record of bhray_trace_rays_records: two 16-byte halves (the kernel stores words 0-3 as one float4, word 4 alone, words 5-7 in the epilogue)
SZ(bhray_ray_record, 32);
OFF(bhray_ray_record, position, 0); OFF(bhray_ray_record, hit, 12); OFF(bhray_ray_record, triangle, 16); OFF(bhray_ray_record, iterations, 20);
OFF(bhray_ray_record, closest, 24); OFF(bhray_ray_record, transmittance, 28);
// a point of bhray_trace_rays_paths: one 16-byte store of the path kernels
SZ(bhray_path_point, 16);
OFF(bhray_path_point, position, 0); OFF(bhray_path_point, iteration, 12);
// the parameters and the report of bhray_accum_add_adaptive
SZ(bhray_accum_adaptive, 24);
OFF(bhray_accum_adaptive, struct_size, 0); OFF(bhray_accum_adaptive, min_samples, 4); OFF(bhray_accum_adaptive, max_samples, 8); OFF(bhray_accum_adaptive, round_samples, 12);
OFF(bhray_accum_adaptive, tolerance, 16); OFF(bhray_accum_adaptive, dark, 20);
SZ(bhray_accum_adaptive_info, 24);
OFF(bhray_accum_adaptive_info, rounds, 0); OFF(bhray_accum_adaptive_info, active_last, 4); OFF(bhray_accum_adaptive_info, rays, 8); OFF(bhray_accum_adaptive_info, reach, 16);
// the still camera of bhray_accum_set_camera
SZ(bhray_still_camera, 20);
OFF(bhray_still_camera, struct_size, 0); OFF(bhray_still_camera, projection, 4); OFF(bhray_still_camera, fisheye_fov, 8); OFF(bhray_still_camera, lens_radius, 12);
OFF(bhray_still_camera, focus_distance, 16);
static_assert(BHRAY_STILL_PINHOLE == 0 && BHRAY_STILL_EQUIRECT == 1 && BHRAY_STILL_FISHEYE == 2, "BHRAY_STILL_*");
// the still filter of bhray_accum_set_filter
SZ(bhray_still_filter, 20);
OFF(bhray_still_filter, struct_size, 0); OFF(bhray_still_filter, kind, 4); OFF(bhray_still_filter, radius, 8); OFF(bhray_still_filter, b, 12); OFF(bhray_still_filter, c, 16);
static_assert(BHRAY_FILTER_BOX == 0 && BHRAY_FILTER_TENT == 1 && BHRAY_FILTER_CUBIC == 2, "BHRAY_FILTER_*");
// a star and the parameters of bhray_set_stars; the per-pixel report of bhray_diag_stars_pixel_info_host
SZ(bhray_star, 24);
OFF(bhray_star, dir, 0); OFF(bhray_star, flux, 12);
SZ(bhray_star_params, 16);
OFF(bhray_star_params, struct_size, 0); OFF(bhray_star_params, gain, 4); OFF(bhray_star_params, min_area, 8); OFF(bhray_star_params, max_footprint, 12);
SZ(bhray_star_pixel_info, 32);
OFF(bhray_star_pixel_info, state, 0); OFF(bhray_star_pixel_info, tested, 12); OFF(bhray_star_pixel_info, area, 24);
static_assert(BHRAY_MAX_STARS == (1u << 22) && BHRAY_STARS_MAX_CELLS == 64u, "BHRAY_MAX_STARS / BHRAY_STARS_MAX_CELLS");
// the moving observer of bhray_accum_set_observer
SZ(bhray_observer, 20);
OFF(bhray_observer, struct_size, 0); OFF(bhray_observer, velocity, 4); OFF(bhray_observer, beaming, 16);
static_assert(BHRAY_OBSERVER_MAX_SPEED2 == 0.9801f, "BHRAY_OBSERVER_MAX_SPEED2");
static_assert(BHRAY_MAX_PATH_STRIDE_LOG2 == 16&& BHRAY_MAX_PATH_POINTS_PER_CALL == (1u << 24), "BHRAY_MAX_PATH_*");
static_assert(BHRAY_HIT_NONE == 0 && BHRAY_HIT_HORIZON == 1 && BHRAY_HIT_DISK == 2 && BHRAY_HIT_MESH == 3 && BHRAY_HIT_UNUSABLE == 255, "BHRAY_HIT_*");
// the still passes of bhray_accum_set_passes: one bit and one sum plane each
static_assert(BHRAY_PASS_COVERAGE == 1 && BHRAY_PASS_GEOMETRY == 2 && BHRAY_PASS_POSITION == 4 && BHRAY_PASS_ESCAPE == 8 && BHRAY_PASS_ALL == 15, "BHRAY_PASS_*");
// the parameters of the denoised stills
static_assert(sizeof(bhray_still_denoise) == 32, "bhray_still_denoise");
OFF(bhray_still_denoise, struct_size, 0); OFF(bhray_still_denoise, iterations, 4); OFF(bhray_still_denoise, guides, 8); OFF(bhray_still_denoise, sigma_colour, 12); OFF(bhray_still_denoise, sigma_escape, 28);
static_assert(BHRAY_DENOISE_MAX_ITERATIONS == 5u, "BHRAY_DENOISE_MAX_ITERATIONS");

// not reference layouts, but ABI the bindings restate (bhusie_amd/layouts.py)
static_assert(sizeof(bhray_counters) == 104, "bhray_counters");
static_assert(BHRAY_COMM_ID_BYTES == 128, "ncclUniqueId");
OFF(bhray_config, level_w, 12); OFF(bhray_config, level_h, 12 + 4 * BHRAY_MAX_LEVELS); OFF(bhray_config, crop_x, 12 + 8 * BHRAY_MAX_LEVELS);
OFF(bhray_config, superset_levels, 12 + 8 * BHRAY_MAX_LEVELS + 44);
OFF(bhray_config, device_count, 12 + 8 * BHRAY_MAX_LEVELS + 48);
OFF(bhray_config, devices, 12 + 8 * BHRAY_MAX_LEVELS + 52);
OFF(bhray_config, gather, 12 + 8 * BHRAY_MAX_LEVELS + 52 + 4 * BHRAY_MAX_DEVICES);
OFF(bhray_config, comm_id, 12 + 8 * BHRAY_MAX_LEVELS + 52 + 4 * BHRAY_MAX_DEVICES + 8);
OFF(bhray_config, partition, 12 + 8 * BHRAY_MAX_LEVELS + 52 + 4 * BHRAY_MAX_DEVICES + 8 + BHRAY_COMM_ID_BYTES);
OFF(bhray_config, slab_row0, 12 + 8 * BHRAY_MAX_LEVELS + 52 + 4 * BHRAY_MAX_DEVICES + 8 + BHRAY_COMM_ID_BYTES + 4);
SZ(bhray_config, 12 + 8 * BHRAY_MAX_LEVELS + 52 + 4 * BHRAY_MAX_DEVICES + 8 + BHRAY_COMM_ID_BYTES + 4 + 4 * (BHRAY_MAX_DEVICES + 1));
SZ(bhray_level_grid_info, 12 * BHRAY_LEVEL_GRID_LAUNCHES + 24 + 16);
OFF(bhray_level_grid_info, total_launches, 8 * BHRAY_LEVEL_GRID_LAUNCHES); OFF(bhray_level_grid_info, blocks, 8 * BHRAY_LEVEL_GRID_LAUNCHES + 24);
OFF(bhray_level_grid_info, enabled, 12 * BHRAY_LEVEL_GRID_LAUNCHES + 24);

// The persistent grid of one ladder trace launch from the rays its queues held the last time (bhray_diag.h): enough blocks to hold the expected rays
// plus a margin in `rays_per_block_generation` rays per block, at least one block per frame of the batch (blockIdx % frames picks a block's own frame) and at least
// `floor_blocks`, never more than the ctx's grid.  Scheduling only: the waves of a trace launch are persistent and pull until every queue of the batch is exhausted,
// so an estimate that is too small - a scene cut - costs that launch time and no pixel; the floor bounds how much.  Pure host arithmetic, in 64 bits: the sum of 32 frames'
// 32-bit queue lengths is below 2^37, the margin is capped at 1000 %, so nothing overflows.
extern "C" uint32_t bhray_trace_grid_for(uint64_t expected_rays, uint32_t frames_in_batch, uint32_t ctx_grid, uint32_t rays_per_block_generation,
                                         uint32_t margin_percent, uint32_t floor_blocks) {
    if (expected_rays == BHRAY_LEVEL_GRID_NO_FEEDBACK || rays_per_block_generation == 0) return ctx_grid;    // nothing to size from: the ctx's grid
    if (expected_rays > ((uint64_t)1 << 40)) return ctx_grid;                                                  // (no sum of 32-bit queue lengths gets here)
    if (margin_percent > 1000u) margin_percent = 1000u;
    const uint64_t with_margin = (expected_rays * (100ull + (uint64_t)margin_percent) + 99ull) / 100ull;
    uint64_t blocks = (with_margin + rays_per_block_generation - 1) / rays_per_block_generation;
    const uint64_t lo = frames_in_batch > floor_blocks ? frames_in_batch : floor_blocks;
    if (blocks < lo) blocks = lo;
    if (blocks > ctx_grid) blocks = ctx_grid;                                                                  // the ceiling wins: no launch gets a larger grid than before
    return (uint32_t)blocks;
}
