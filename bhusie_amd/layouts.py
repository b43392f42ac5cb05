"""ctypes mirrors of include/bhray.h (which mirrors the reference's #[repr(C)] structs) and include/bhray_diag.h."""
from __future__ import annotations

import ctypes as C

MAX_LEVELS = 8
MAX_DEVICES = 16
COMM_ID_BYTES = 128
GATHER_NONE, GATHER_RCCL = 0, 1
PARTITION_STRIPES, PARTITION_SLABS = 0, 1
MAX_MODEL_VERTICES = 524288
MAX_MODELS = 8                       # BHRAY_MAX_MODELS: model slots per ctx (ray.wgsl:2 raised from 1)
MODEL_UNIFORM_BYTES = 48234572
F_COUNTERS = 1
F_TIMING = 2
F_LITERAL = 4
F_TEMPORAL = 8
F_TIMING_SPARSE = 16
F_EVAL_FMA = 32
F_GATHER_SKY = 128
TEX_TEMP_LUT, TEX_DISK, TEX_SKY = 0, 1, 2
FXAA_MAX_ITERATIONS = 1024
MAX_RAYS_PER_CALL = 1 << 26          # BHRAY_MAX_RAYS_PER_CALL
ACCUM_MAX_SAMPLES = 65536            # BHRAY_ACCUM_MAX_SAMPLES


class BhrayError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"bhray error {code}: {msg}")
        self.code = code


class BhrayDetails(C.Structure):            # ray_pipeline.rs:3-14
    _fields_ = [("material_count", C.c_int32), ("model_count", C.c_int32), ("time", C.c_float),
                ("integration_method", C.c_int32), ("step_size", C.c_float), ("max_iterations", C.c_int32),
                ("angle_division_threshold", C.c_float), ("highlight_interpolation", C.c_int32)]


class BhrayCameraUniform(C.Structure):      # camera.rs:66-73
    _fields_ = [("position", C.c_float * 3), ("_padding", C.c_uint32), ("forward", C.c_float * 3), ("fov", C.c_float)]


class BhrayBlackHoleUniform(C.Structure):   # blackhole.rs:37-51
    _fields_ = [("accretion_disk_inner", C.c_float), ("accretion_disk_outer", C.c_float),
                ("rotation_speed", C.c_float), ("relativity_sphere_radius", C.c_float),
                ("position", C.c_float * 3), ("show_disk_texture", C.c_int32),
                ("normal", C.c_float * 3), ("show_red_shift", C.c_int32),
                ("rotation_matrix", C.c_float * 12), ("feather_amount", C.c_float), ("pad", C.c_int32 * 8)]


class BhrayBlackHole(C.Structure):          # blackhole.rs:3-13
    _fields_ = [("position", C.c_float * 3), ("accretion_disk_rotation", C.c_float * 3),
                ("accretion_disk_inner", C.c_float), ("accretion_disk_outer", C.c_float),
                ("rotation_speed", C.c_float), ("relativity_sphere_radius", C.c_float),
                ("show_disk_texture", C.c_int32), ("show_red_shift", C.c_int32), ("feather_amount", C.c_float)]


class BhrayNode(C.Structure):               # triangle.rs:45-52
    _fields_ = [("min_corner", C.c_float * 3), ("left_child", C.c_int32), ("max_corner", C.c_float * 3), ("obj_count", C.c_int32)]


class BhrayTriangle(C.Structure):           # triangle.rs:54-63
    _fields_ = [(n, C.c_int32) for n in ("p1", "p2", "p3", "n1", "n2", "n3")]


class BhrayFxaaDetails(C.Structure):       # fxaa_pipline.rs:76-83 (FXAADetailsUniform)
    _fields_ = [("edge_threshold_min", C.c_float), ("edge_threshold_max", C.c_float), ("iterations", C.c_int32), ("subpixel_quality", C.c_float)]


class BhrayMixDetails(C.Structure):         # mix_pipeline.rs:5-7 (MixDetails)
    _fields_ = [("mix_ratio", C.c_float)]


class BhrayRay(C.Structure):                # bhray_ray: one ray of bhray_trace_rays, two 16-byte halves
    _fields_ = [("origin", C.c_float * 3), ("pad0", C.c_float), ("direction", C.c_float * 3), ("pad1", C.c_float)]


class BhrayRayRecord(C.Structure):          # bhray_ray_record: what bhray_trace_rays_records knows about one ray, two 16-byte halves
    _fields_ = [("position", C.c_float * 3), ("hit", C.c_uint32), ("triangle", C.c_int32), ("iterations", C.c_uint32),
                ("closest", C.c_float), ("transmittance", C.c_float)]


class BhrayPathPoint(C.Structure):          # bhray_path_point: one sample of a ray's path (bhray_trace_rays_paths), 16 bytes
    _fields_ = [("position", C.c_float * 3), ("iteration", C.c_uint32)]


# bhray_path_point as a NumPy structured type (numpy is imported here only for this: the package's other array types live in renderer.py / model.py)
import numpy as _np  # noqa: E402
PATH_POINT_DTYPE = _np.dtype([("position", _np.float32, 3), ("iteration", _np.uint32)])
assert PATH_POINT_DTYPE.itemsize == C.sizeof(BhrayPathPoint) == 16
MAX_PATH_STRIDE_LOG2 = 16                   # BHRAY_MAX_PATH_STRIDE_LOG2
MAX_PATH_POINTS_PER_CALL = 1 << 24          # BHRAY_MAX_PATH_POINTS_PER_CALL
HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH, HIT_UNUSABLE = 0, 1, 2, 3, 255      # BHRAY_HIT_*: bits 0-7 of bhray_ray_record.hit (bits 8-15: the model slot of a MESH hit)
LENS_FRAMES, LENS_RAYS = 1, 2                                                   # BHRAY_LENS_*: the bits of bhray_set_mesh_lensing's `on` (frames; also ray batches, records and stills)


class BhrayAccumAdaptive(C.Structure):      # bhray_accum_adaptive: the parameters of bhray_accum_add_adaptive
    _fields_ = [("struct_size", C.c_uint32), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("round_samples", C.c_uint32),
                ("tolerance", C.c_float), ("dark", C.c_float)]


class BhrayAccumAdaptiveInfo(C.Structure):  # bhray_accum_adaptive_info: what one bhray_accum_add_adaptive call did
    _fields_ = [("rounds", C.c_uint32), ("active_last", C.c_uint32), ("rays", C.c_uint64), ("reach", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


assert C.sizeof(BhrayAccumAdaptive) == 24 and C.sizeof(BhrayAccumAdaptiveInfo) == 24 and BhrayAccumAdaptiveInfo.rays.offset == 8

STILL_PINHOLE, STILL_EQUIRECT, STILL_FISHEYE = 0, 1, 2      # BHRAY_STILL_*


class BhrayStillCamera(C.Structure):        # bhray_still_camera: the accumulation image's camera (bhray_accum_set_camera)
    _fields_ = [("struct_size", C.c_uint32), ("projection", C.c_uint32), ("fisheye_fov", C.c_float), ("lens_radius", C.c_float), ("focus_distance", C.c_float)]


assert C.sizeof(BhrayStillCamera) == 20 and BhrayStillCamera.focus_distance.offset == 16

FILTER_BOX, FILTER_TENT, FILTER_CUBIC = 0, 1, 2             # BHRAY_FILTER_*
PASS_COVERAGE, PASS_GEOMETRY, PASS_POSITION, PASS_ESCAPE, PASS_ALL = 1, 2, 4, 8, 0xF     # BHRAY_PASS_*: the still passes (bhray_accum_set_passes)
PASS_NAMES = {"coverage": PASS_COVERAGE, "geometry": PASS_GEOMETRY, "position": PASS_POSITION, "escape": PASS_ESCAPE}


class BhrayStillFilter(C.Structure):        # bhray_still_filter: the accumulation image's reconstruction filter (bhray_accum_set_filter)
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("radius", C.c_float), ("b", C.c_float), ("c", C.c_float)]


assert C.sizeof(BhrayStillFilter) == 20 and BhrayStillFilter.c.offset == 16


class BhrayStillDenoise(C.Structure):       # bhray_still_denoise: the parameters of a denoised read of the accumulation image (bhray_accum_read_denoised)
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("guides", C.c_uint32), ("sigma_colour", C.c_float), ("sigma_coverage", C.c_float),
                ("sigma_closest", C.c_float), ("sigma_position", C.c_float), ("sigma_escape", C.c_float)]


assert C.sizeof(BhrayStillDenoise) == 32 and BhrayStillDenoise.sigma_escape.offset == 28
DENOISE_MAX_ITERATIONS = 5                  # BHRAY_DENOISE_MAX_ITERATIONS


class BhrayObserver(C.Structure):           # bhray_observer: the moving observer of a still (bhray_accum_set_observer)
    _fields_ = [("struct_size", C.c_uint32), ("velocity", C.c_float * 3), ("beaming", C.c_uint32)]


assert C.sizeof(BhrayObserver) == 20 and BhrayObserver.beaming.offset == 16
OBSERVER_MAX_SPEED2 = 0.9801                # BHRAY_OBSERVER_MAX_SPEED2

MAX_STARS, STARS_MAX_CELLS = 1 << 22, 64                    # BHRAY_MAX_STARS, BHRAY_STARS_MAX_CELLS


class BhrayStar(C.Structure):               # bhray_star: a point source of the catalogue (bhray_set_stars)
    _fields_ = [("dir", C.c_float * 3), ("flux", C.c_float * 3)]


class BhrayStarParams(C.Structure):         # bhray_star_params; BhrayStarParams.default() is bhray_star_params_default's
    _fields_ = [("struct_size", C.c_uint32), ("gain", C.c_float), ("min_area", C.c_float), ("max_footprint", C.c_float)]

    @classmethod
    def default(cls, **kw):
        p = cls(C.sizeof(cls), 1.0, 1e-7, 0.25)
        for k, v in kw.items():
            setattr(p, k, v)
        return p


assert C.sizeof(BhrayStar) == 24 and BhrayStar.flux.offset == 12
assert C.sizeof(BhrayStarParams) == 16 and BhrayStarParams.max_footprint.offset == 12


class BhrayModelDesc(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("visible", C.c_int32),
                ("points", C.c_void_p), ("normals", C.c_void_p), ("triangles", C.c_void_p),
                ("nodes", C.c_void_p), ("bvh_lookup", C.c_void_p),
                ("point_count", C.c_int32), ("normal_count", C.c_int32), ("triangle_count", C.c_int32), ("node_count", C.c_int32)]


class BhrayConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("levels", C.c_uint32),
                ("level_w", C.c_uint32 * MAX_LEVELS), ("level_h", C.c_uint32 * MAX_LEVELS),
                ("crop_x", C.c_uint32), ("crop_y", C.c_uint32), ("frame_w", C.c_uint32), ("frame_h", C.c_uint32),
                ("row_rank", C.c_uint32), ("row_world", C.c_uint32), ("stripe_rows", C.c_uint32), ("flags", C.c_uint32),
                ("frames_in_flight", C.c_uint32), ("speculative_levels", C.c_uint32), ("frames_per_batch", C.c_uint32),
                ("superset_levels", C.c_uint32), ("device_count", C.c_uint32), ("devices", C.c_int32 * MAX_DEVICES), ("gather", C.c_uint32),
                ("gather_root", C.c_uint32), ("comm_id", C.c_uint8 * COMM_ID_BYTES),
                ("partition", C.c_uint32), ("slab_row0", C.c_uint32 * (MAX_DEVICES + 1))]

    def sizes(self):
        return [(int(self.level_w[i]), int(self.level_h[i])) for i in range(self.levels)]


class BhrayCounters(C.Structure):
    FRAME = ("pixels", "copied", "interpolated", "traced", "steps", "flat_iters", "node_pairs", "triangles", "disk_hits", "sky_samples")
    SCHED = ("wave_steps", "rays_adopted", "max_ray_iterations")
    _fields_ = [(n, C.c_uint64) for n in FRAME + SCHED]

    def as_dict(self):
        """the counters that are a property of the frame (equal to the oracle's)"""
        return {n: int(getattr(self, n)) for n in self.FRAME}

    def scheduling(self):
        """how the trace kernel scheduled that work: depends on the build, frames in flight, batches"""
        d = {n: int(getattr(self, n)) for n in self.SCHED}
        d["step_lane_occupancy"] = (self.steps / (64.0 * self.wave_steps)) if self.wave_steps else None
        return d


class BhrayTiming(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("batches", C.c_uint32), ("total_ms", C.c_float), ("trace_ms", C.c_float), ("classify_ms", C.c_float),
                ("trace_launches", C.c_uint32), ("classify_launches", C.c_uint32),
                ("level_trace_ms", C.c_float * MAX_LEVELS), ("level_classify_ms", C.c_float * MAX_LEVELS),
                ("sky_ms", C.c_float), ("sky_launches", C.c_uint32),
                ("gather_ms", C.c_float), ("deinterleave_ms", C.c_float), ("gathers", C.c_uint32),
                ("predicted_trace_ms", C.c_float), ("predicted_launches", C.c_uint32),
                ("trace_exec_ms", C.c_float), ("trace_exec_launches", C.c_uint32)]


class BhrayGatherInfo(C.Structure):
    _fields_ = [("partitions", C.c_uint32), ("local_partitions", C.c_uint32), ("root", C.c_uint32), ("root_is_local", C.c_uint32),
                ("comm_ranks", C.c_uint32), ("rccl_version", C.c_uint32),
                ("bytes_sent_per_frame", C.c_uint64), ("bytes_received_per_frame", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BhrayModelBuildInfo(C.Structure):
    """bhray_model_build_info (include/bhray_diag.h)"""
    _fields_ = [(n, C.c_uint32) for n in ("built_on_device", "triangles", "nodes", "leaves", "max_leaf", "max_depth")] + \
               [("upload_ms", C.c_float), ("build_ms", C.c_float)]

    def as_dict(self):
        return {n: (float if t is C.c_float else int)(getattr(self, n)) for n, t in self._fields_}


assert C.sizeof(BhrayDetails) == 32 and C.sizeof(BhrayCameraUniform) == 32 and C.sizeof(BhrayBlackHoleUniform) == 132
assert C.sizeof(BhrayNode) == 32 and C.sizeof(BhrayTriangle) == 24
assert C.sizeof(BhrayRay) == 32 and BhrayRay.direction.offset == 16
assert C.sizeof(BhrayPathPoint) == 16 and BhrayPathPoint.iteration.offset == 12
assert C.sizeof(BhrayRayRecord) == 32 and BhrayRayRecord.hit.offset == 12 and BhrayRayRecord.triangle.offset == 16 and BhrayRayRecord.transmittance.offset == 28

LEVEL_GRID_LAUNCHES = MAX_LEVELS + 2
LEVEL_GRID_NO_FEEDBACK = 2 ** 64 - 1


class BhrayLevelGridInfo(C.Structure):
    """bhray_level_grid_info (include/bhray_diag.h): trace grids sized by queue length.  Launch ids: 0 the speculative levels' merged launch, 1 + l level l,
    MAX_LEVELS + 1 the superset launch."""
    _fields_ = [("expected_rays", C.c_uint64 * LEVEL_GRID_LAUNCHES), ("total_launches", C.c_uint64), ("total_blocks", C.c_uint64), ("total_ceiling_launches", C.c_uint64),
                ("blocks", C.c_uint32 * LEVEL_GRID_LAUNCHES), ("enabled", C.c_uint32), ("frames", C.c_uint32), ("ctx_grid", C.c_uint32), ("dense", C.c_uint32)]

    def as_dict(self):
        """launches: {id: (blocks, expected rays or None)} of the trace launches the batch had"""
        return {"enabled": bool(self.enabled), "frames": int(self.frames), "ctx_grid": int(self.ctx_grid), "dense": bool(self.dense),
                "launches": {i: (int(self.blocks[i]), None if int(self.expected_rays[i]) == LEVEL_GRID_NO_FEEDBACK else int(self.expected_rays[i]))
                             for i in range(LEVEL_GRID_LAUNCHES) if int(self.blocks[i])},
                "total_launches": int(self.total_launches), "total_blocks": int(self.total_blocks), "total_ceiling_launches": int(self.total_ceiling_launches)}


assert C.sizeof(BhrayLevelGridInfo) == 12 * LEVEL_GRID_LAUNCHES + 40


class BhrayRebalanceInfo(C.Structure):
    """bhray_rebalance_info (include/bhray.h)"""
    _fields_ = [("partitions", C.c_uint32), ("applied", C.c_uint32), ("slab_row0", C.c_uint32 * 17), ("part_cost", C.c_float * 16), ("extra_cost", C.c_float * 16),
                ("slowest_before", C.c_float), ("slowest_predicted", C.c_float), ("frames", C.c_uint32)]

    def as_dict(self):
        n = int(self.partitions)
        return {"partitions": n, "applied": bool(self.applied), "slab_row0": [int(v) for v in self.slab_row0[:n + 1]], "part_cost": [float(v) for v in self.part_cost[:n]],
                "extra_cost": [float(v) for v in self.extra_cost[:n]], "slowest_before": float(self.slowest_before), "slowest_predicted": float(self.slowest_predicted),
                "frames": int(self.frames)}


P = C.POINTER
vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int32, C.c_size_t
# every symbol include/bhray.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "bhray_ladder_from_base": (C.c_int, [u32, u32, u32, u32, P(BhrayConfig)]),
    "bhray_ladder_for_frame": (C.c_int, [u32, u32, u32, u32, P(BhrayConfig)]),
    "bhray_create": (C.c_int, [P(BhrayConfig), P(vp)]),
    "bhray_destroy": (None, [vp]),
    "bhray_last_error": (C.c_char_p, [vp]),
    "bhray_strerror": (C.c_char_p, [C.c_int]),
    "bhray_version": (u32, []),
    "bhray_device_count": (C.c_int, []),
    "bhray_partition_rows": (u32, [u32, u32, u32, u32]),
    "bhray_partition_row_index": (C.c_int, [u32, u32, u32, u32, u32, P(u32)]),
    "bhray_config_partition_rows": (u32, [P(BhrayConfig), u32]),
    "bhray_config_partition_row_index": (C.c_int, [P(BhrayConfig), u32, u32, P(u32)]),
    "bhray_balance_slabs": (C.c_int, [P(BhrayConfig), P(P(C.c_uint64)), u32, P(u32)]),
    "bhray_comm_unique_id": (C.c_int, [vp]),
    "bhray_set_partition": (C.c_int, [vp, P(u32)]),
    "bhray_get_partition": (C.c_int, [vp, P(u32), P(u32)]),
    "bhray_rebalance_slabs": (C.c_int, [u32, u32, P(u32), P(C.c_double), P(C.c_double), C.c_double, P(C.c_double), P(u32), P(C.c_double)]),
    "bhray_rebalance": (C.c_int, [vp, P(BhrayRebalanceInfo)]),
    "bhray_get_work": (C.c_int, [vp, P(C.c_double), P(C.c_double), P(u32)]),
    "bhray_get_partition_costs": (C.c_int, [vp, P(C.c_double), P(C.c_double), P(u32)]),
    "bhray_set_materials": (C.c_int, [vp, vp, sz]),
    "bhray_set_texture": (C.c_int, [vp, C.c_int, vp, u32, u32]),
    "bhray_upload_model_uniform": (C.c_int, [vp, u32, vp, sz]),
    "bhray_upload_model": (C.c_int, [vp, u32, P(BhrayModelDesc)]),
    "bhray_upload_model_build": (C.c_int, [vp, u32, P(BhrayModelDesc)]),
    "bhray_update_model_vertices": (C.c_int, [vp, u32, vp, i32, vp, i32]),
    "bhray_update_model_vertices_device": (C.c_int, [vp, u32, vp, i32, vp, i32, vp]),
    "bhray_set_model_pose": (C.c_int, [vp, u32, P(C.c_float)]),
    "bhray_pose_from_euler": (C.c_int, [P(C.c_float), P(C.c_float), C.c_float, P(C.c_float)]),
    "bhray_set_model_transform": (C.c_int, [vp, u32, P(C.c_float), i32]),
    "bhray_set_uniforms": (C.c_int, [vp, vp, vp, vp]),
    "bhray_set_mesh_lensing": (C.c_int, [vp, i32]),
    "bhray_trace_rays": (C.c_int, [vp, P(BhrayRay), u32, P(C.c_float)]),
    "bhray_trace_rays_device": (C.c_int, [vp, vp, u32, vp, vp]),
    "bhray_trace_rays_sky": (C.c_int, [vp, P(BhrayRay), u32, P(C.c_float), vp]),
    "bhray_trace_rays_records": (C.c_int, [vp, P(BhrayRay), u32, P(C.c_float), P(BhrayRayRecord)]),
    "bhray_trace_rays_records_device": (C.c_int, [vp, vp, u32, vp, vp, vp]),
    "bhray_trace_rays_paths": (C.c_int, [vp, P(BhrayRay), u32, u32, u32, P(C.c_float), P(BhrayRayRecord), P(BhrayPathPoint), P(C.c_uint32)]),
    "bhray_trace_rays_paths_device": (C.c_int, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]),
    "bhray_accum_begin": (C.c_int, [vp]),
    "bhray_accum_add": (C.c_int, [vp, u32]),
    "bhray_accum_samples": (C.c_int, [vp, P(u32)]),
    "bhray_accum_read": (C.c_int, [vp, vp, sz]),
    "bhray_accum_read_display": (C.c_int, [vp, vp, sz]),
    "bhray_accum_sample_offset": (None, [u32, P(C.c_float), P(C.c_float)]),
    "bhray_accum_add_adaptive": (C.c_int, [vp, P(BhrayAccumAdaptive), P(BhrayAccumAdaptiveInfo)]),
    "bhray_accum_read_counts": (C.c_int, [vp, vp, sz]),
    "bhray_accum_set_camera": (C.c_int, [vp, P(BhrayStillCamera)]),
    "bhray_still_camera_default": (None, [P(BhrayStillCamera)]),
    "bhray_accum_set_filter": (C.c_int, [vp, P(BhrayStillFilter)]),
    "bhray_still_filter_default": (None, [P(BhrayStillFilter)]),
    "bhray_accum_filter_weights": (C.c_int, [P(BhrayStillFilter), u32, P(C.c_float), P(C.c_float)]),
    "bhray_render": (C.c_int, [vp]),
    "bhray_flush": (C.c_int, [vp]),
    "bhray_sync": (C.c_int, [vp]),
    "bhray_read_hdr": (C.c_int, [vp, vp, sz]),
    "bhray_local_rows": (u32, [vp]),
    "bhray_local_row_index": (C.c_int, [vp, u32, P(u32)]),
    "bhray_hdr_device_ptr": (C.c_int, [vp, P(vp), P(sz)]),
    "bhray_bind_output": (C.c_int, [vp, vp, sz]),
    "bhray_read_hdr_async": (C.c_int, [vp, vp, sz, P(C.c_uint64)]),
    "bhray_read_sky_async": (C.c_int, [vp, vp, sz, P(C.c_uint64)]),
    "bhray_wait_read": (C.c_int, [vp, C.c_uint64]),
    "bhray_host_alloc": (C.c_int, [sz, P(vp)]),
    "bhray_host_free": (C.c_int, [vp]),
    "bhray_import_external_fd": (C.c_int, [vp, C.c_int, sz, P(vp)]),
    "bhray_release_external": (C.c_int, [vp, vp]),
    "bhray_resolve_sky": (C.c_int, [vp]),
    "bhray_read_sky": (C.c_int, [vp, vp, sz]),
    "bhray_sky_device_ptr": (C.c_int, [vp, P(vp), P(sz)]),
    "bhray_set_sky_filter": (C.c_int, [vp, i32]),
    "bhray_sky_pyramid_sizes": (C.c_int, [u32, u32, P(u32), P(u32), P(u32)]),
    "bhray_star_params_default": (None, [P(BhrayStarParams)]),
    "bhray_set_stars": (C.c_int, [vp, vp, u32, P(BhrayStarParams)]),
    "bhray_star_grid_size": (C.c_int, [u32, P(u32)]),
    "bhray_star_cell": (C.c_int, [P(C.c_float), u32, P(u32)]),
    "bhray_stars_resolve_host": (C.c_int, [vp, u32, u32, vp, u32, P(BhrayStarParams), vp]),
    "bhray_accum_set_stars": (C.c_int, [vp, i32]),
    "bhray_accum_stars_resolve_host": (C.c_int, [vp, u32, u32, i32, vp, u32, P(BhrayStarParams), vp]),
    "bhray_accum_set_observer": (C.c_int, [vp, P(BhrayObserver)]),
    "bhray_accum_set_passes": (C.c_int, [vp, u32]),
    "bhray_accum_passes": (C.c_int, [vp, P(u32)]),
    "bhray_accum_read_pass": (C.c_int, [vp, u32, vp, sz]),
    "bhray_accum_pass_values": (C.c_int, [vp, vp, vp, u32, u32, vp]),
    "bhray_still_denoise_default": (None, [P(BhrayStillDenoise)]),
    "bhray_accum_read_denoised": (C.c_int, [vp, P(BhrayStillDenoise), vp, sz]),
    "bhray_accum_read_display_denoised": (C.c_int, [vp, P(BhrayStillDenoise), vp, sz]),
    "bhray_accum_denoise_host": (C.c_int, [vp, P(vp), u32, u32, P(BhrayStillDenoise), vp]),
    "bhray_observer_default": (None, [P(BhrayObserver)]),
    "bhray_observer_boost_rays": (C.c_int, [P(BhrayObserver), vp, u32, vp, vp]),
    "bhray_post_defaults": (C.c_int, [P(BhrayFxaaDetails), P(BhrayMixDetails)]),
    "bhray_bloom_sizes": (C.c_int, [u32, u32, P(u32), P(u32)]),
    "bhray_set_post_uniforms": (C.c_int, [vp, vp, vp]),
    "bhray_resolve_display": (C.c_int, [vp]),
    "bhray_read_display": (C.c_int, [vp, vp, sz]),
    "bhray_read_display_async": (C.c_int, [vp, vp, sz, P(C.c_uint64)]),
    "bhray_display_device_ptr": (C.c_int, [vp, P(vp), P(sz)]),
    "bhray_wait_stream": (C.c_int, [vp, vp]),
    "bhray_signal_stream": (C.c_int, [vp, vp]),
    "bhray_next_stream": (C.c_int, [vp, P(vp)]),
    "bhray_camera_uniform_update": (None, [P(BhrayCameraUniform), P(C.c_float), P(C.c_float), C.c_float]),
    "bhray_black_hole_default": (None, [P(BhrayBlackHole)]),
    "bhray_black_hole_uniform_update": (None, [P(BhrayBlackHoleUniform), P(BhrayBlackHole)]),
    "bhray_details_default": (None, [P(BhrayDetails)]),
    "bhray_model_new": (C.c_int, [P(vp)]),
    "bhray_model_free": (None, [vp]),
    "bhray_model_add_vertex": (C.c_int, [vp, P(C.c_float)]),
    "bhray_model_add_normal": (C.c_int, [vp, P(C.c_float)]),
    "bhray_model_add_triangle": (C.c_int, [vp, P(BhrayTriangle)]),
    "bhray_model_build_bvh": (C.c_int, [vp]),
    "bhray_model_max_depth": (C.c_int, [vp]),
    "bhray_model_build_bvh_sah": (C.c_int, [vp]),
    "bhray_model_desc_get": (C.c_int, [vp, P(BhrayModelDesc)]),
    "bhray_model_set_transform": (C.c_int, [vp, P(C.c_float), i32]),
    "bhray_model_pack_uniform": (C.c_int, [vp, vp, sz]),
    "bhray_load_model": (C.c_int, [C.c_char_p, P(vp)]),
    "bhray_generate_disk_texture": (C.c_int, [u32, vp]),
}

# every symbol include/bhray_diag.h declares (measurement and verification): name -> (restype, argtypes)
DIAG_SYMBOLS = {
    "bhray_get_counters": (C.c_int, [vp, P(BhrayCounters)]),
    "bhray_get_level_counters": (C.c_int, [vp, u32, P(BhrayCounters)]),
    "bhray_get_row_work": (C.c_int, [vp, u32, P(C.c_uint64), u32]),
    "bhray_get_timing": (C.c_int, [vp, P(BhrayTiming)]),
    "bhray_selftest": (C.c_int, [vp, P(C.c_uint64)]),
    "bhray_get_trace_builds": (C.c_int, [vp, P(C.c_uint64)]),
    "bhray_get_err_skip": (C.c_int, [vp, P(C.c_uint64)]),
    "bhray_trace_grid_for": (u32, [C.c_uint64, u32, u32, u32, u32, u32]),
    "bhray_get_level_grids": (C.c_int, [vp, u32, P(BhrayLevelGridInfo)]),
    "bhray_read_level": (C.c_int, [vp, u32, vp, sz]),
    "bhray_get_gather_info": (C.c_int, [vp, P(BhrayGatherInfo)]),
    "bhray_get_model_build_info": (C.c_int, [vp, u32, P(BhrayModelBuildInfo)]),
    "bhray_read_model_bvh": (C.c_int, [vp, u32, vp, u32, vp, u32, P(u32), P(u32)]),
    "bhray_read_model_vertices": (C.c_int, [vp, u32, vp, u32, vp, u32, P(u32), P(u32)]),
    "bhray_accum_sample_rays": (C.c_int, [vp, u32, P(BhrayRay)]),
    "bhray_accum_denoise_times": (C.c_int, [vp, P(BhrayStillDenoise), P(C.c_float)]),
    "bhray_accum_set_launch_rays": (C.c_int, [vp, u32]),
    "bhray_still_sample_rays_host": (C.c_int, [P(BhrayConfig), vp, P(BhrayStillCamera), u32, P(BhrayRay)]),
    "bhray_observer_sample_rays_host": (C.c_int, [P(BhrayConfig), vp, P(BhrayStillCamera), P(BhrayObserver), u32, vp, vp]),
    "bhray_accum_active_pixels": (C.c_int, [vp, P(BhrayAccumAdaptive), P(u32), u32, P(u32)]),
    "bhray_read_sky_pyramid_level": (C.c_int, [vp, u32, vp, sz]),
    "bhray_diag_display_image": (C.c_int, [C.c_int, vp, u32, u32, vp, vp, u32, vp, vp, sz]),
    "bhray_diag_star_image": (C.c_int, [vp, vp, u32, u32, vp, vp]),
    "bhray_diag_stars_pixel_info_host": (C.c_int, [vp, u32, u32, vp, u32, P(BhrayStarParams), vp]),
}
DIAG_DISPLAY_FXAA_ONLY = 1           # BHRAY_DIAG_DISPLAY_FXAA_ONLY


def declare(L):
    import os
    old_build = os.environ.get("BHRAY_AB_OLD_BUILD") == "1"      # kernel A/B against a library built from an earlier tree (profiles/jobs/ab.sh): symbols it lacks are not bound
    for name, (res, args) in {**SYMBOLS, **DIAG_SYMBOLS}.items():
        if old_build and not hasattr(L, name):
            continue
        f = getattr(L, name)          # AttributeError if the library does not export it
        f.restype = res
        f.argtypes = args


def check(rc, ctx=None, L=None):
    """Raise BhrayError for a non-zero return code; the message comes from the library the ctx belongs to (L)."""
    if rc != 0:
        if L is None:
            from ._lib import lib
            L = lib()
        msg = L.bhray_last_error(ctx) or b""
        if not msg:
            msg = L.bhray_strerror(rc)
        raise BhrayError(rc, msg.decode("utf-8", "replace"))
