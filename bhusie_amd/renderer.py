"""RayPass / Renderer — the Python mirror of the reference's ray-pass surface.

RayPass   = the chain of RayPipelines (src/renderer/pipelines/ray_pipeline.rs:28-310) as one
            object over a bhray_ctx: textures, model, per-frame uniforms, dispatch, output.
Renderer  = the part of Renderer::{new,render} on the path (src/renderer/mod.rs:113-207,
            378-420): default RayDetails, the 72x41 x3 x4 ladder, per-frame call order.
All pixels come from libbhray (gfx950); nothing is computed here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib
from .layouts import (BhrayFxaaDetails, BhrayMixDetails, DIAG_DISPLAY_FXAA_ONLY, MAX_MODELS, PARTITION_SLABS, F_COUNTERS, F_EVAL_FMA, F_GATHER_SKY, F_LITERAL, F_TEMPORAL, F_TIMING, F_TIMING_SPARSE, GATHER_RCCL, TEX_DISK, TEX_SKY, TEX_TEMP_LUT, BhrayConfig, BhrayCounters, BhrayRay, BhrayRayRecord, BhrayPathPoint, PATH_POINT_DTYPE, HIT_MESH, HIT_UNUSABLE, LENS_FRAMES, LENS_RAYS,
                      BhrayAccumAdaptive, BhrayAccumAdaptiveInfo, BhrayStar, BhrayStarParams, BhrayStillFilter, BhrayStillDenoise, FILTER_BOX, FILTER_TENT, FILTER_CUBIC, PASS_COVERAGE, PASS_GEOMETRY, PASS_POSITION, PASS_ESCAPE, PASS_ALL, PASS_NAMES,
                      BhrayGatherInfo, BhrayModelBuildInfo, BhrayModelDesc, BhrayRebalanceInfo, BhrayTiming, check)
from .model import NODE_DTYPE, Model
from .scene import BlackHole, Camera, RayDetails
from .cameras import pinhole_rays

# bhray_ray_record as a NumPy structured type (32 bytes: layouts.BhrayRayRecord)
RAY_RECORD_DTYPE = np.dtype([("position", np.float32, 3), ("hit", np.uint32), ("triangle", np.int32), ("iterations", np.uint32),
                             ("closest", np.float32), ("transmittance", np.float32)])
assert RAY_RECORD_DTYPE.itemsize == C.sizeof(BhrayRayRecord) == 32


class AdaptiveStill:
    """The parameters of an adaptive still (Renderer.render_still(adaptive=...), RayPass.accum_add_adaptive)."""

    def __init__(self, min_samples: int = 4, max_samples: int = 64, round_samples: int = 4, tolerance: float = 0.05, dark: float = 0.01):
        self.min_samples, self.max_samples, self.round_samples = int(min_samples), int(max_samples), int(round_samples)
        self.tolerance, self.dark = float(tolerance), float(dark)

    def as_kwargs(self) -> dict:
        return {"min_samples": self.min_samples, "max_samples": self.max_samples, "round_samples": self.round_samples, "tolerance": self.tolerance, "dark": self.dark}


class StillFilter:
    """The reconstruction filter of a still (Renderer.render_still(filter=...), RayPass.accum_set_filter; bhray_still_filter): StillFilter.tent(radius),
    StillFilter.mitchell(radius) (B = C = 1/3), StillFilter.bspline(radius) (B = 1, C = 0), or StillFilter(FILTER_CUBIC, radius, b, c); radius is the support's half
    width in pixels.  StillFilter() is the box.  A cubic with c > 0 has negative lobes: a mean may be slightly negative."""

    def __init__(self, kind: int = FILTER_BOX, radius: float = 2.0, b: float = 1.0 / 3.0, c: float = 1.0 / 3.0):
        self.kind, self.radius, self.b, self.c = int(kind), float(radius), float(b), float(c)

    @classmethod
    def tent(cls, radius: float = 1.0) -> "StillFilter":
        return cls(FILTER_TENT, radius)

    @classmethod
    def mitchell(cls, radius: float = 2.0) -> "StillFilter":
        return cls(FILTER_CUBIC, radius, 1.0 / 3.0, 1.0 / 3.0)

    @classmethod
    def bspline(cls, radius: float = 2.0) -> "StillFilter":
        return cls(FILTER_CUBIC, radius, 1.0, 0.0)

    def struct(self) -> BhrayStillFilter:
        """the bhray_still_filter the library takes"""
        return BhrayStillFilter(C.sizeof(BhrayStillFilter), self.kind, self.radius, self.b, self.c)

    def weights(self, s: int):
        """(wx, wy): the five horizontal and five vertical weights of sample s (bhray_accum_filter_weights: host arithmetic), float32"""
        wx, wy = np.zeros(5, np.float32), np.zeros(5, np.float32)
        st = self.struct()
        check(lib().bhray_accum_filter_weights(C.byref(st), int(s), wx.ctypes.data_as(C.POINTER(C.c_float)), wy.ctypes.data_as(C.POINTER(C.c_float))))
        return wx, wy

    def __repr__(self):
        return f"StillFilter(kind={self.kind}, radius={self.radius}, b={self.b}, c={self.c})"


class StillDenoise:
    """The parameters of a denoised read of a still (Renderer.render_still(denoise=...), RayPass.accum_read_denoised; bhray_still_denoise): an
    edge-avoiding a-trous filter of `iterations` levels (1 .. 5: tap spacing 1, 2, 4, 8, 16 pixels) over the colour mean, guided by the still's passes.  guides: 0 -
    every pass the still carries - or a non-empty subset of them (PASS_* bits).  Each sigma is the difference at which a tap's weight reaches zero: of the compressed
    luminance, of the coverage vector, of the closest approach, of the premultiplied hit position and of the escape vector.  A sigma left None takes the library's
    default (bhray_still_denoise_default), and so does iterations."""

    def __init__(self, iterations: int | None = None, guides: int = 0, sigma_colour: float | None = None, sigma_coverage: float | None = None,
                 sigma_closest: float | None = None, sigma_position: float | None = None, sigma_escape: float | None = None):
        d = BhrayStillDenoise()
        lib().bhray_still_denoise_default(C.byref(d))
        self.iterations = int(d.iterations if iterations is None else iterations)
        self.guides = int(guides)
        self.sigma_colour = float(d.sigma_colour if sigma_colour is None else sigma_colour)
        self.sigma_coverage = float(d.sigma_coverage if sigma_coverage is None else sigma_coverage)
        self.sigma_closest = float(d.sigma_closest if sigma_closest is None else sigma_closest)
        self.sigma_position = float(d.sigma_position if sigma_position is None else sigma_position)
        self.sigma_escape = float(d.sigma_escape if sigma_escape is None else sigma_escape)

    def struct(self) -> BhrayStillDenoise:
        """the bhray_still_denoise the library takes"""
        return BhrayStillDenoise(C.sizeof(BhrayStillDenoise), self.iterations, self.guides, self.sigma_colour, self.sigma_coverage, self.sigma_closest,
                                 self.sigma_position, self.sigma_escape)

    def __repr__(self):
        return (f"StillDenoise(iterations={self.iterations}, guides={self.guides}, sigma_colour={self.sigma_colour}, sigma_coverage={self.sigma_coverage}, "
                f"sigma_closest={self.sigma_closest}, sigma_position={self.sigma_position}, sigma_escape={self.sigma_escape})")


def _denoise_struct(denoise):
    """None (the library's defaults), True (the same), a StillDenoise or a BhrayStillDenoise -> the struct to pass, or None"""
    if denoise is None or denoise is True:
        return None
    return denoise.struct() if hasattr(denoise, "struct") else denoise


def ladder_from_base(base=(72, 41), multiplier=3, levels=4) -> BhrayConfig:
    cfg = BhrayConfig()
    check(lib().bhray_ladder_from_base(base[0], base[1], multiplier, levels, C.byref(cfg)))
    return cfg


def ladder_for_frame(frame=(1920, 1080), multiplier=3, levels=4) -> BhrayConfig:
    cfg = BhrayConfig()
    check(lib().bhray_ladder_for_frame(frame[0], frame[1], multiplier, levels, C.byref(cfg)))
    return cfg


def post_defaults():
    """(BhrayFxaaDetails, BhrayMixDetails): the display pass's uniforms as Renderer::render uploads them (bhray_post_defaults)."""
    f, m = BhrayFxaaDetails(), BhrayMixDetails()
    check(lib().bhray_post_defaults(C.byref(f), C.byref(m)))
    return f, m


def bloom_sizes(frame_w: int, frame_h: int):
    """[(w, h)] of the 10 bloom targets (5 down, 5 up) of a frame_w x frame_h frame (bhray_bloom_sizes: host arithmetic)."""
    w, h = (C.c_uint32 * 10)(), (C.c_uint32 * 10)()
    check(lib().bhray_bloom_sizes(int(frame_w), int(frame_h), w, h))
    return [(int(a), int(b)) for a, b in zip(w, h)]


def display_image(sky16, fxaa=None, mix=None, device=0, fxaa_only=False, stages=False):
    """The display pass over a supplied RGBA16F image (bhray_diag_display_image: the launches resolve_display runs, no ctx): sky16 is
    (H, W, 4) float16 or its uint16 words; fxaa / mix are the uniform blocks as RayPass.set_post_uniforms takes them.  Returns the
    uint8 (H, W, 4) image; with stages=True also the nine intermediate bloom levels [(h_i, w_i, 4) uint16] and the tone-mapped
    (H, W, 4) uint16 image.  fxaa_only: sky16 is taken as the tone-mapped image and only FXAA and the RGBA8 store run."""
    a = np.asarray(sky16)
    if a.dtype != np.float16 and a.dtype != np.uint16:
        raise TypeError("display_image takes binary16 pixels (float16, or their uint16 words)")
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("display_image takes an (H, W, 4) image")
    a = np.ascontiguousarray(a)
    h, w = a.shape[:2]
    f = bytes(fxaa) if fxaa is not None else None
    m = bytes(BhrayMixDetails(float(mix))) if isinstance(mix, (int, float, np.floating)) else (bytes(mix) if mix is not None else None)
    assert (f is None or len(f) == 16) and (m is None or len(m) == 4)
    out = np.empty((h, w, 4), dtype=np.uint8)
    buf, texels = None, 0
    if stages:
        sizes = bloom_sizes(w, h)[:9]
        texels = sum(lw * lh for lw, lh in sizes) + w * h
        buf = np.empty((texels, 4), dtype=np.uint16)
    check(lib().bhray_diag_display_image(int(device), a.ctypes.data, w, h, f, m, DIAG_DISPLAY_FXAA_ONLY if fxaa_only else 0, out.ctypes.data,
                                         buf.ctypes.data if buf is not None else None, texels))
    if not stages:
        return out
    levels, at = [], 0
    for lw, lh in sizes:
        levels.append(buf[at:at + lw * lh].reshape(lh, lw, 4))
        at += lw * lh
    return out, levels, buf[at:].reshape(h, w, 4)


def sky_pyramid_sizes(w: int, h: int):
    """[(w, h)] of the levels of the sky filter's pyramid over a w x h texture, level 0 (the texture) included (bhray_sky_pyramid_sizes: host arithmetic)."""
    n, lw, lh = C.c_uint32(), (C.c_uint32 * 32)(), (C.c_uint32 * 32)()
    check(lib().bhray_sky_pyramid_sizes(int(w), int(h), C.byref(n), lw, lh))
    return [(int(lw[i]), int(lh[i])) for i in range(n.value)]


def star_array(stars):
    """(a, n): a catalogue as the library takes it - a C-contiguous (n, 6) float32 array, rows (dir x y z, flux r g b), the bytes of n bhray_star.  Takes None, an
    (n, 6) array, or a ctypes array of layouts.BhrayStar."""
    if stars is None:
        return np.zeros((0, 6), np.float32), 0
    if isinstance(stars, C.Array) and getattr(stars, "_type_", None) is BhrayStar:
        stars = np.frombuffer(stars, dtype=np.float32).reshape(-1, 6)
    a = np.ascontiguousarray(stars, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError("a star catalogue is an (n, 6) array: dir x y z, flux r g b")
    return a, int(a.shape[0])


def star_grid_size(n: int) -> int:
    """G of the catalogue index of n stars (bhray_star_grid_size: host arithmetic)."""
    g = C.c_uint32()
    check(lib().bhray_star_grid_size(int(n), C.byref(g)))
    return int(g.value)


def star_cells(dirs, G: int) -> np.ndarray:
    """The index cell of every direction of an (n, 3) array in a grid of side G (bhray_star_cell: host arithmetic), uint32."""
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.empty(len(d), np.uint32)
    L, c = lib(), C.c_uint32()
    for i in range(len(d)):
        check(L.bhray_star_cell(d[i].ctypes.data_as(C.POINTER(C.c_float)), int(G), C.byref(c)))
        out[i] = c.value
    return out


def stars_resolve_host(frame, stars, params=None) -> np.ndarray:
    """The star pass's per-pixel rule over an (h, w, 4) float32 frame on the host (bhray_stars_resolve_host, no device): (h, w, 4) float32, what each pixel
    receives (times the gain) and, in alpha, the number of stars it accepted."""
    f = np.ascontiguousarray(frame, dtype=np.float32)
    a, n = star_array(stars)
    out = np.empty_like(f)
    check(lib().bhray_stars_resolve_host(f.ctypes.data, f.shape[1], f.shape[0], a.ctypes.data, n, C.byref(params) if params is not None else None, out.ctypes.data))
    return out


def accum_stars_resolve_host(results, stars, params=None, wrap_x=False) -> np.ndarray:
    """stars_resolve_host over a still's sample image (bhray_accum_stars_resolve_host, DESIGN.md §24, no device): with wrap_x the image is periodic in x - column -1 is
    column w - 1 and column w is column 0 -, as a whole equirect still's."""
    f = np.ascontiguousarray(results, dtype=np.float32)
    a, n = star_array(stars)
    out = np.empty_like(f)
    check(lib().bhray_accum_stars_resolve_host(f.ctypes.data, f.shape[1], f.shape[0], int(bool(wrap_x)), a.ctypes.data, n, C.byref(params) if params is not None else None,
                                               out.ctypes.data))
    return out


def accum_pass_values(results, records, rays, pass_bit: int) -> np.ndarray:
    """What every sample contributes to one still pass (bhray_accum_pass_values, DESIGN.md §27: host arithmetic through the function the kernels call, no device):
    (n, 4) float32 - (v, 1) for a taken sample, zeros for a skipped one.  results: (n, 4) trace results; records: n records of RAY_RECORD_DTYPE; rays: (n, 8), read
    for PASS_ESCAPE only (None otherwise).  pass_bit: exactly one PASS_* bit (BhrayError otherwise)."""
    r = np.ascontiguousarray(results, dtype=np.float32).reshape(-1, 4)
    q = np.ascontiguousarray(records, dtype=RAY_RECORD_DTYPE).reshape(-1)
    d = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8) if rays is not None else None
    if q.shape[0] != r.shape[0] or (d is not None and d.shape[0] != r.shape[0]):
        raise ValueError("accum_pass_values: results, records and rays must hold the same number of samples")
    out = np.empty_like(r)
    check(lib().bhray_accum_pass_values(r.ctypes.data, q.ctypes.data, d.ctypes.data if d is not None else None, r.shape[0], int(pass_bit), out.ctypes.data))
    return out


def accum_denoise_host(colour, guides, denoise=None) -> np.ndarray:
    """The denoiser's rule on the host (bhray_accum_denoise_host, DESIGN.md §28: host arithmetic through the functions the kernels call, no device).  colour: the
    (h, w, 4) float32 colour mean; guides: {PASS_* bit: (h, w, 4) float32 pass mean} - the planes present are the set; denoise: a StillDenoise or None (the defaults).
    Returns the (h, w, 4) float32 denoised mean.  BhrayError where the parameters are refused."""
    c = np.ascontiguousarray(colour, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 4:
        raise ValueError("accum_denoise_host: colour must be (h, w, 4)")
    planes, keep = (C.c_void_p * 4)(), []
    for bit, g in dict(guides).items():
        bit = int(bit)
        if bit not in (PASS_COVERAGE, PASS_GEOMETRY, PASS_POSITION, PASS_ESCAPE):
            raise ValueError(f"accum_denoise_host: {bit} is not one PASS_* bit")
        a = np.ascontiguousarray(g, dtype=np.float32)
        if a.shape != c.shape:
            raise ValueError("accum_denoise_host: a guide plane must have the colour's shape")
        keep.append(a)
        planes[bit.bit_length() - 1] = a.ctypes.data
    st = _denoise_struct(denoise)
    out = np.empty_like(c)
    check(lib().bhray_accum_denoise_host(c.ctypes.data, planes, c.shape[1], c.shape[0], C.byref(st) if st is not None else None, out.ctypes.data))
    return out


STAR_PIXEL_INFO_DTYPE = np.dtype([("state", np.uint32), ("faces", np.uint32), ("cells", np.uint32), ("tested", np.uint32), ("accepted", np.uint32),
                                  ("reversed", np.uint32), ("area", np.float32), ("pad", np.uint32)])


def stars_pixel_info_host(frame, stars, params=None) -> np.ndarray:
    """What the rule did at every pixel (bhray_diag_stars_pixel_info_host): an (h, w) array of STAR_PIXEL_INFO_DTYPE."""
    f = np.ascontiguousarray(frame, dtype=np.float32)
    a, n = star_array(stars)
    out = np.empty(f.shape[:2], STAR_PIXEL_INFO_DTYPE)
    check(lib().bhray_diag_stars_pixel_info_host(f.ctypes.data, f.shape[1], f.shape[0], a.ctypes.data, n, C.byref(params) if params is not None else None, out.ctypes.data))
    return out


def pose_from_euler(rotation, pivot=(0.0, 0.0, 0.0), scale=1.0) -> np.ndarray:
    """The (3, 4) float32 pose [A | t] of RayPass.set_model_pose for a rotation (Euler angles, BlackHole's convention) about `pivot` with a uniform
    scale: A = R * scale, t = pivot - A pivot (bhray_pose_from_euler: host arithmetic)."""
    out = (C.c_float * 12)()
    check(lib().bhray_pose_from_euler((C.c_float * 3)(*[float(x) for x in rotation]), (C.c_float * 3)(*[float(x) for x in pivot]), float(scale), out))
    return np.array(out, dtype=np.float32).reshape(3, 4)


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (one process per GPU: call on ONE rank, hand the bytes to every rank's RayPass)."""
    buf = (C.c_uint8 * 128)()
    check(lib().bhray_comm_unique_id(buf))
    return bytes(buf)


def partition_rows(frame_h: int, world: int, stripe_rows: int = 27):
    """rows[part] = frame rows of every partition, from the library's own partition arithmetic (host only)."""
    L = lib()
    out, r = [], C.c_uint32()
    for part in range(world):
        n = int(L.bhray_partition_rows(frame_h, world, stripe_rows, part))
        rows = np.zeros(n, dtype=np.int64)
        for i in range(n):
            check(L.bhray_partition_row_index(frame_h, world, stripe_rows, part, i, C.byref(r)))
            rows[i] = r.value
        out.append(rows)
    return out


def config_partition_rows(cfg: BhrayConfig):
    """rows[part] for the partition a config describes (stripes or slabs)."""
    L = lib()
    world = cfg.device_count if cfg.device_count >= 2 else max(1, cfg.row_world)
    out, r = [], C.c_uint32()
    for part in range(world):
        n = int(L.bhray_config_partition_rows(C.byref(cfg), part))
        rows = np.zeros(n, dtype=np.int64)
        for i in range(n):
            check(L.bhray_config_partition_row_index(C.byref(cfg), part, i, C.byref(r)))
            rows[i] = r.value
        out.append(rows)
    return out


def balance_slabs(cfg: BhrayConfig, row_work, world: int):
    """slab_row0[0..world] that minimise the largest partition's work; row_work[l] = per-row work of ladder level l of a calibration
    frame rendered whole (RayPass.row_work()) - bhray_balance_slabs, pure host arithmetic."""
    assert len(row_work) == cfg.levels
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in row_work]
    for l, a in enumerate(arrs):
        assert a.shape == (cfg.level_h[l],), (l, a.shape)
    ptrs = (C.POINTER(C.c_uint64) * cfg.levels)(*[a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in arrs])
    out = (C.c_uint32 * (world + 1))()
    check(lib().bhray_balance_slabs(C.byref(cfg), ptrs, world, out))
    return [int(v) for v in out]


def rebalance_slabs(frame_h: int, slab_row0, part_ms, row_weight: np.ndarray, extra_ms=None, shift_rows: float = 0.0):
    """bhray_rebalance_slabs: (new bounds, predicted slowest partition); row_weight (float64[frame_h], zeros before the first call) is updated in place."""
    world = len(part_ms)
    if len(slab_row0) != world + 1:
        raise ValueError(f"rebalance_slabs: {world} partitions need {world + 1} bounds, got {len(slab_row0)}")
    if extra_ms is not None and len(extra_ms) != world:
        raise ValueError(f"rebalance_slabs: extra_ms has {len(extra_ms)} entries for {world} partitions")
    assert row_weight.dtype == np.float64 and row_weight.shape == (frame_h,) and row_weight.flags.c_contiguous
    b_in = (C.c_uint32 * (world + 1))(*[int(v) for v in slab_row0])
    ms = (C.c_double * world)(*[float(v) for v in part_ms])
    ex = (C.c_double * world)(*[float(v) for v in extra_ms]) if extra_ms is not None else None
    out = (C.c_uint32 * (world + 1))()
    pred = C.c_double()
    check(lib().bhray_rebalance_slabs(frame_h, world, b_in, ms, ex, float(shift_rows), row_weight.ctypes.data_as(C.POINTER(C.c_double)), out, C.byref(pred)))
    return [int(v) for v in out], float(pred.value)


class RayPass:
    """devices=[d0, d1, ...]: ONE ctx drives several GPUs (partition i on devices[i]); bhray_render then also gathers the row
    tiles to `gather_root`'s GPU over RCCL and de-interleaves them, and every output call refers to the whole frame.
    comm_id + row_rank/row_world: one process per GPU, the same gather enqueued by every rank's library."""

    def __init__(self, cfg: BhrayConfig, device=0, counters=False, timing=False, row_rank=0, row_world=1, stripe_rows=27,
                 frames_in_flight=0, speculative_levels=0, frames_per_batch=0, devices=None, gather_root=0, comm_id=None,
                 literal=False, superset_levels=0, temporal=False, eval_fma=False, slab_row0=None, gather_sky=False):
        cfg = BhrayConfig.from_buffer_copy(bytes(cfg))
        cfg.struct_size = C.sizeof(BhrayConfig)
        cfg.device = device
        if devices is not None:
            cfg.device_count = len(devices)                      # more than BHRAY_MAX_DEVICES: refused by bhray_create
            for i, d in enumerate(list(devices)[:len(cfg.devices)]):
                cfg.devices[i] = int(d)
        cfg.gather_root = gather_root
        if comm_id is not None:
            assert len(comm_id) == 128
            cfg.gather = GATHER_RCCL
            C.memmove(cfg.comm_id, bytes(comm_id), 128)
        cfg.flags = (F_COUNTERS if counters else 0) | (F_TIMING_SPARSE if timing == "sparse" else (F_TIMING if timing else 0)) | (F_LITERAL if literal else 0) | (F_TEMPORAL if temporal else 0) | (F_EVAL_FMA if eval_fma else 0) | (F_GATHER_SKY if gather_sky else 0)
        cfg.row_rank, cfg.row_world, cfg.stripe_rows = row_rank, row_world, stripe_rows
        if slab_row0 is not None:                                # contiguous slabs instead of interleaved stripes (bhray_config.partition)
            cfg.partition = PARTITION_SLABS
            for i, v in enumerate(list(slab_row0)[:len(cfg.slab_row0)]):
                cfg.slab_row0[i] = int(v)
        cfg.frames_in_flight = frames_in_flight
        cfg.speculative_levels = speculative_levels
        cfg.frames_per_batch = frames_per_batch
        cfg.superset_levels = superset_levels
        self.cfg = cfg
        h = C.c_void_p()
        self._L = lib()                                          # the library this ctx belongs to: EVERY call on self._h goes through it (a handle of one .so must never be driven by another)
        check(self._L.bhray_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.bhray_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- static inputs
    def set_texture(self, slot: int, rgba: np.ndarray):
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4
        check(self._L.bhray_set_texture(self._h, slot, a.ctypes.data, a.shape[1], a.shape[0]), self._h, self._L)

    def set_textures(self, temp_lut, disk, sky):
        self.set_texture(TEX_TEMP_LUT, temp_lut); self.set_texture(TEX_DISK, disk); self.set_texture(TEX_SKY, sky)

    def upload_model(self, model: Model, index=0):
        d = model.desc()
        check(self._L.bhray_upload_model(self._h, index, C.byref(d)), self._h, self._L)

    def upload_model_build(self, model, index=0):
        """Points, normals and triangles of `model` (a Model, or a dict shaped like Model.arrays(): its nodes / bvh_lookup are not read);
        the tree is built on the GPU (bhray_upload_model_build)."""
        if isinstance(model, Model):
            d = model.desc()
        else:
            keep = [np.ascontiguousarray(model["points"], dtype=np.float32), np.ascontiguousarray(model["normals"], dtype=np.float32),
                    np.ascontiguousarray(model["triangles"], dtype=np.int32)]
            assert keep[0].ndim == 2 and keep[0].shape[1] == 4 and keep[1].ndim == 2 and keep[1].shape[1] == 4 and keep[2].ndim == 2 and keep[2].shape[1] == 6
            d = BhrayModelDesc()
            d.position = (C.c_float * 3)(*[float(x) for x in model.get("position", (0.0, 0.0, 0.0))])
            d.visible = int(model.get("visible", 1))
            d.points, d.normals, d.triangles = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data
            d.point_count, d.normal_count, d.triangle_count = len(keep[0]), len(keep[1]), len(keep[2])
        check(self._L.bhray_upload_model_build(self._h, index, C.byref(d)), self._h, self._L)

    def update_model_vertices(self, points=None, normals=None, index=0):
        """New points and / or normals ((n, 4) float32, the counts the slot holds) for a slot built by upload_model_build; the tree is rebuilt
        on the GPU in the slot's own buffers (bhray_update_model_vertices)."""
        p = np.ascontiguousarray(points, dtype=np.float32) if points is not None else None
        n = np.ascontiguousarray(normals, dtype=np.float32) if normals is not None else None
        for a in (p, n):
            assert a is None or (a.ndim == 2 and a.shape[1] == 4)
        check(self._L.bhray_update_model_vertices(self._h, index, p.ctypes.data if p is not None else None, len(p) if p is not None else 0,
                                                  n.ctypes.data if n is not None else None, len(n) if n is not None else 0), self._h, self._L)

    def update_model_vertices_device(self, d_points, d_normals, point_count, normal_count, stream=None, index=0):
        """update_model_vertices with the arrays in device memory: d_points / d_normals are device pointers (int; None keeps that array) to point_count /
        normal_count float4s; the copies are ordered behind everything enqueued so far on hipStream_t `stream` (None: the legacy stream).  The call
        synchronises, so the source may be overwritten once it returns (bhray_update_model_vertices_device)."""
        check(self._L.bhray_update_model_vertices_device(self._h, index, C.c_void_p(d_points) if d_points else None, int(point_count) if d_points else 0,
                                                         C.c_void_p(d_normals) if d_normals else None, int(normal_count) if d_normals else 0,
                                                         C.c_void_p(stream) if stream else None), self._h, self._L)

    def set_model_pose(self, pose, index=0):
        """Affine pose of a slot built by upload_model_build, applied to its rest geometry on the GPU; the tree is rebuilt there (bhray_set_model_pose,
        DESIGN.md §14).  pose: 12 floats, row-major 3x4 [A | t] (pose_from_euler makes one), always relative to the rest arrays; None: back to them."""
        if pose is None:
            m = None
        else:
            a = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1)
            assert a.size == 12
            m = (C.c_float * 12)(*[float(x) for x in a])
        check(self._L.bhray_set_model_pose(self._h, index, m), self._h, self._L)

    def read_model_vertices(self, index=0) -> dict:
        """dict(points, normals): the (n, 4) float32 arrays the kernels read for slot `index` now - posed, if a pose is in force (bhray_read_model_vertices)"""
        np_, nn = C.c_uint32(), C.c_uint32()
        check(self._L.bhray_read_model_vertices(self._h, index, None, 0, None, 0, C.byref(np_), C.byref(nn)), self._h, self._L)      # the counts
        points, normals = np.zeros((np_.value, 4), dtype=np.float32), np.zeros((nn.value, 4), dtype=np.float32)
        check(self._L.bhray_read_model_vertices(self._h, index, points.ctypes.data, np_.value, normals.ctypes.data, nn.value, C.byref(np_), C.byref(nn)), self._h, self._L)
        return dict(points=points, normals=normals)

    def read_model_bvh(self, index=0) -> dict:
        """dict(nodes, bvh_lookup) - the shape of Model.arrays() - of the tree slot `index` holds on the device, in the device's numbering."""
        nn, nt = C.c_uint32(), C.c_uint32()
        self._L.bhray_read_model_bvh(self._h, index, None, 0, None, 0, C.byref(nn), C.byref(nt))      # sizes first (BHRAY_E_INVALID unless both are 0)
        nodes, lookup = np.zeros(nn.value, dtype=NODE_DTYPE), np.zeros(nt.value, dtype=np.int32)
        check(self._L.bhray_read_model_bvh(self._h, index, nodes.ctypes.data, nn.value, lookup.ctypes.data, nt.value, C.byref(nn), C.byref(nt)), self._h, self._L)
        return dict(nodes=nodes, bvh_lookup=lookup)

    def model_build_info(self, index=0) -> dict:
        """built_on_device, triangles, nodes, leaves, max_leaf, max_depth, upload_ms, build_ms of slot `index` (bhray_get_model_build_info)"""
        info = BhrayModelBuildInfo()
        check(self._L.bhray_get_model_build_info(self._h, index, C.byref(info)), self._h, self._L)
        return info.as_dict()

    def upload_model_uniform(self, blob: bytes, index=0):
        check(self._L.bhray_upload_model_uniform(self._h, index, blob, len(blob)), self._h, self._L)

    def set_materials(self, blob: bytes = bytes(128)):
        """mod.rs:389 — accepted and ignored (the shader never reads the materials)."""
        check(self._L.bhray_set_materials(self._h, blob, len(blob)), self._h, self._L)

    def row_work(self):
        """[per-row iterations of the last render, one uint64 array per ladder level] (needs counters=True) - the input of balance_slabs."""
        out = []
        for l in range(self.cfg.levels):
            a = np.zeros(self.cfg.level_h[l], dtype=np.uint64)
            check(self._L.bhray_get_row_work(self._h, l, a.ctypes.data_as(C.POINTER(C.c_uint64)), a.size), self._h, self._L)
            out.append(a)
        return out

    def gather_info(self) -> dict:
        g = BhrayGatherInfo()
        check(self._L.bhray_get_gather_info(self._h, C.byref(g)), self._h, self._L)
        return g.as_dict()

    # -- run-time partition (multi-GPU balance that follows the scene)
    def set_partition(self, slab_row0):
        """From the next render on partition p owns frame rows [slab_row0[p], slab_row0[p + 1]) - no re-create (bhray_set_partition)."""
        parts = int(self.cfg.device_count) if self.cfg.device_count >= 2 else max(1, int(self.cfg.row_world))
        if len(slab_row0) != parts + 1:                     # the library reads partitions + 1 entries whatever it is handed
            raise ValueError(f"set_partition: {parts} partitions need {parts + 1} bounds, got {len(slab_row0)}")
        a = (C.c_uint32 * (parts + 1))(*[int(v) for v in slab_row0])
        check(self._L.bhray_set_partition(self._h, a), self._h, self._L)

    def get_partition(self):
        a, n = (C.c_uint32 * 17)(), C.c_uint32()
        check(self._L.bhray_get_partition(self._h, a, C.byref(n)), self._h, self._L)
        return [int(v) for v in a[:n.value + 1]]

    def work(self):
        """(integrator steps the trace waves issued, pixels the classify launches visited) per frame, over the frames the slots still hold (bhray_get_work)"""
        ws, px, n = C.c_double(), C.c_double(), C.c_uint32()
        check(self._L.bhray_get_work(self._h, C.byref(ws), C.byref(px), C.byref(n)), self._h, self._L)
        return float(ws.value), float(px.value), int(n.value)

    def partition_costs(self):
        """(cost[partitions], extra[partitions]) of the partitions this ctx renders - bhray_rebalance's own numbers (bhray_get_partition_costs)"""
        n = int(self.cfg.device_count) if self.cfg.device_count >= 2 else max(1, int(self.cfg.row_world))
        cost, extra = (C.c_double * n)(), (C.c_double * n)()
        check(self._L.bhray_get_partition_costs(self._h, cost, extra, None), self._h, self._L)
        return [float(v) for v in cost], [float(v) for v in extra]

    def rebalance(self) -> dict:
        """New slab bounds from the work the ctx's kernels counted for the frames in its slots; applied when they promise >= 2 % (bhray_rebalance)."""
        info = BhrayRebalanceInfo()
        check(self._L.bhray_rebalance(self._h, C.byref(info)), self._h, self._L)
        return info.as_dict()

    def set_model_transform(self, position, visible=1, index=0):
        check(self._L.bhray_set_model_transform(self._h, index, (C.c_float * 3)(*[float(x) for x in position]), int(visible)), self._h, self._L)

    def set_mesh_lensing(self, on):
        """Lensed meshes (bhray_set_mesh_lensing): from the next render on, models are also tested on every integrator step inside the
        relativity sphere.  Off by default; BhrayError (BHRAY_E_STATE) for on on a literal / eval_fma ctx.  `on` is True / False (LENS_FRAMES / 0), or the
        setting's word: an integer >= 2 is passed through - LENS_FRAMES | LENS_RAYS lenses the ray batches, the records and the stills as well."""
        word = int(on) if isinstance(on, (int, np.integer)) and not isinstance(on, bool) and int(on) >= 2 else (1 if on else 0)
        check(self._L.bhray_set_mesh_lensing(self._h, word), self._h, self._L)

    # -- ray batches (bhray_trace_rays)
    @staticmethod
    def _ray_records(rays) -> np.ndarray:
        """(n, 6) origin + direction or (n, 8) records -> contiguous (n, 8) float32 (layouts.BhrayRay)"""
        r = np.asarray(rays, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] not in (6, 8):
            raise ValueError(f"trace_rays: rays must be (n, 6) or (n, 8) float32, got {r.shape}")
        if r.shape[1] == 8:
            return np.ascontiguousarray(r)
        out = np.zeros((r.shape[0], 8), dtype=np.float32)
        out[:, 0:3] = r[:, 0:3]; out[:, 4:7] = r[:, 3:6]
        return out

    def trace_rays(self, rays, sky: bool = False):
        """What the shader's trace_ray returns for each ray under the ctx's current uniforms, textures and models: (n, 4) float32, (colour, 1) or
        (escape direction, 0).  A non-finite component or an all-zero direction: BhrayError (BHRAY_E_INVALID).  sky=True: also the RGBA16F image of the
        sky pass over the results, returned as a pair (bhray_trace_rays_sky)."""
        rec = self._ray_records(rays)
        n = rec.shape[0]
        out = np.zeros((n, 4), dtype=np.float32)
        rp = rec.ctypes.data_as(C.POINTER(BhrayRay)) if n else None
        op = out.ctypes.data_as(C.POINTER(C.c_float)) if n else None
        if not sky:
            check(self._L.bhray_trace_rays(self._h, rp, n, op), self._h, self._L)
            return out
        out16 = np.zeros((n, 4), dtype=np.float16)
        check(self._L.bhray_trace_rays_sky(self._h, rp, n, op, out16.ctypes.data if n else None), self._h, self._L)
        return out, out16

    def trace_rays_device(self, d_rays: int, n: int, d_out: int, stream: int | None = None):
        """The device form: n records at device address d_rays -> n RGBA32F results at d_out, enqueued behind what `stream` (a hipStream_t; None: the legacy
        stream) holds now; work enqueued on `stream` afterwards sees the results.  An unusable ray's result is (0, 0, 0, -1) (bhray_trace_rays_device)."""
        check(self._L.bhray_trace_rays_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_out), C.c_void_p(stream) if stream else None), self._h, self._L)

    # -- ray records (bhray_trace_rays_records)
    def trace_rays_records(self, rays):
        """trace_rays, and per ray what trace_ray knew when its loop ended: (results, records) - results as trace_rays, records a structured array
        (RAY_RECORD_DTYPE over the 32 bytes of bhray_ray_record: position, hit, triangle, iterations, closest, transmittance)."""
        rec = self._ray_records(rays)
        n = rec.shape[0]
        out = np.zeros((n, 4), dtype=np.float32)
        records = np.zeros(n, dtype=RAY_RECORD_DTYPE)
        check(self._L.bhray_trace_rays_records(self._h, rec.ctypes.data_as(C.POINTER(BhrayRay)) if n else None, n,
                                               out.ctypes.data_as(C.POINTER(C.c_float)) if n else None,
                                               records.ctypes.data_as(C.POINTER(BhrayRayRecord)) if n else None), self._h, self._L)
        return out, records

    def trace_rays_records_device(self, d_rays: int, n: int, d_out: int, d_records: int, stream: int | None = None):
        """The device form (trace_rays_device's rules): also n records of 32 bytes at the 16-byte aligned device address d_records.  An unusable ray's
        record is hit = HIT_UNUSABLE, triangle = -1, everything else zero (bhray_trace_rays_records_device)."""
        check(self._L.bhray_trace_rays_records_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_out), C.c_void_p(d_records),
                                                      C.c_void_p(stream) if stream else None), self._h, self._L)

    # -- ray paths (bhray_trace_rays_paths)
    def trace_rays_paths(self, rays, stride_log2: int = 0, max_points: int = 1024):
        """trace_rays_records, and per ray the curve the integrator walked, sampled every 2**stride_log2 iterations: (results, records, points, counts) - points an
        (n, max_points) structured array (PATH_POINT_DTYPE: position, iteration), counts (n,) uint32.  Row r holds the origin (iteration 0), the sampled steps and the
        end point - min(counts[r], max_points) points, the rest zero; counts[r] = (iterations >> stride_log2) + 2 whatever max_points is, so counts[r] > max_points says
        that the row is cut short: ask again with a larger stride."""
        rec = self._ray_records(rays)
        n = rec.shape[0]
        out = np.zeros((n, 4), dtype=np.float32)
        records = np.zeros(n, dtype=RAY_RECORD_DTYPE)
        points = np.zeros((n, int(max_points)), dtype=PATH_POINT_DTYPE)
        counts = np.zeros(n, dtype=np.uint32)
        check(self._L.bhray_trace_rays_paths(self._h, rec.ctypes.data_as(C.POINTER(BhrayRay)) if n else None, n, int(stride_log2), int(max_points),
                                             out.ctypes.data_as(C.POINTER(C.c_float)) if n else None,
                                             records.ctypes.data_as(C.POINTER(BhrayRayRecord)) if n else None,
                                             points.ctypes.data_as(C.POINTER(BhrayPathPoint)) if n else None,
                                             counts.ctypes.data_as(C.POINTER(C.c_uint32)) if n else None), self._h, self._L)
        return out, records, points, counts

    def trace_rays_paths_device(self, d_rays: int, n: int, stride_log2: int, max_points: int, d_out: int, d_records: int, d_points: int, d_counts: int,
                                stream: int | None = None):
        """The device form (trace_rays_records_device's rules): also n * max_points points of 16 bytes at the 16-byte aligned device address d_points and n counts at
        d_counts.  Slots behind a ray's last point are not written; an unusable ray gets count 0 and no point (bhray_trace_rays_paths_device)."""
        check(self._L.bhray_trace_rays_paths_device(self._h, C.c_void_p(d_rays), int(n), int(stride_log2), int(max_points), C.c_void_p(d_out), C.c_void_p(d_records),
                                                    C.c_void_p(d_points), C.c_void_p(d_counts), C.c_void_p(stream) if stream else None), self._h, self._L)

    # -- supersampled stills: the accumulation image (bhray_accum_*)
    def accum_begin(self):
        """Clear the accumulation image (allocated on first use); the sample count becomes 0."""
        check(self._L.bhray_accum_begin(self._h), self._h, self._L)

    def accum_add(self, samples: int = 1):
        """Enqueue the next `samples` sub-pixel samples of every frame pixel under the ctx's current uniforms, textures and models: generated, traced, sky-resolved
        and summed on the device.  Returns without waiting.  Before accum_begin, and in the states trace_rays refuses: BhrayError (BHRAY_E_STATE)."""
        check(self._L.bhray_accum_add(self._h, int(samples)), self._h, self._L)

    def accum_samples(self) -> int:
        n = C.c_uint32()
        check(self._L.bhray_accum_samples(self._h, C.byref(n)), self._h, self._L)
        return int(n.value)

    def accum_read(self) -> np.ndarray:
        """The mean of the samples taken so far: (frame_h, frame_w, 4) float32, alpha 1 (0, with a black pixel, where every sample was skipped).  Waits."""
        w, h = int(self.cfg.frame_w), int(self.cfg.frame_h)
        out = np.empty((h, w, 4), dtype=np.float32)
        check(self._L.bhray_accum_read(self._h, out.ctypes.data, w * 16), self._h, self._L)
        return out

    def accum_read_display(self) -> np.ndarray:
        """The mean through the display pass (set_post_uniforms' uniforms): uint8 (frame_h, frame_w, 4) as read_display.  Waits."""
        w, h = int(self.cfg.frame_w), int(self.cfg.frame_h)
        out = np.empty((h, w, 4), dtype=np.uint8)
        check(self._L.bhray_accum_read_display(self._h, out.ctypes.data, w * 4), self._h, self._L)
        return out

    # -- denoised stills: the reads behind an edge-avoiding a-trous filter guided by the passes (bhray_accum_read_denoised)
    def accum_read_denoised(self, denoise=None) -> np.ndarray:
        """accum_read's image denoised: a StillDenoise, or None for the library's defaults.  The accumulation must carry passes (accum_set_passes) and must not be
        adaptive (BhrayError, BHRAY_E_STATE).  Changes no accumulation state: accum_add may continue and accum_read keeps its bits.  Waits."""
        w, h = int(self.cfg.frame_w), int(self.cfg.frame_h)
        out = np.empty((h, w, 4), dtype=np.float32)
        st = _denoise_struct(denoise)
        check(self._L.bhray_accum_read_denoised(self._h, C.byref(st) if st is not None else None, out.ctypes.data, w * 16), self._h, self._L)
        return out

    def accum_denoise_times(self, denoise=None) -> list:
        """The device time of accum_read_denoised's launches in milliseconds, from events (bhray_diag.h): [prepare, a-trous at spacing 1, 2, ...], one entry per
        iteration.  Delivers no image and changes no accumulation state.  Waits."""
        ms = (C.c_float * 6)()
        st = _denoise_struct(denoise)
        check(self._L.bhray_accum_denoise_times(self._h, C.byref(st) if st is not None else None, ms), self._h, self._L)
        n = st.iterations if st is not None else StillDenoise().iterations
        return [float(v) for v in ms[:1 + n]]

    def accum_read_display_denoised(self, denoise=None) -> np.ndarray:
        """accum_read_display's image of the denoised mean: uint8 (frame_h, frame_w, 4).  Waits."""
        w, h = int(self.cfg.frame_w), int(self.cfg.frame_h)
        out = np.empty((h, w, 4), dtype=np.uint8)
        st = _denoise_struct(denoise)
        check(self._L.bhray_accum_read_display_denoised(self._h, C.byref(st) if st is not None else None, out.ctypes.data, w * 4), self._h, self._L)
        return out

    def accum_sample_rays(self, s: int) -> np.ndarray:
        """The records the device generates for sample s under the current uniforms, the still camera and the observer in force: (frame_h * frame_w, 8) float32
        (bhray_diag.h)."""
        out = np.empty((int(self.cfg.frame_w) * int(self.cfg.frame_h), 8), dtype=np.float32)
        check(self._L.bhray_accum_sample_rays(self._h, int(s), out.ctypes.data_as(C.POINTER(BhrayRay))), self._h, self._L)
        return out

    def accum_set_launch_rays(self, max_rays: int = 0):
        """At most max_rays rays per trace launch of accum_add (0: the default, 2**22); the image does not depend on it (bhray_diag.h)."""
        check(self._L.bhray_accum_set_launch_rays(self._h, int(max_rays)), self._h, self._L)

    def accum_set_camera(self, still_camera=None):
        """The camera model of the accumulation image from the next accum_add / accum_add_adaptive on (bhray_accum_set_camera): a cameras.StillCamera
        - .equirect(), .fisheye(fov), .pinhole(lens_radius, focus_distance) - or None for the default, the pinhole without a lens.  Position, forward and the
        pinhole's fov stay those of set_uniforms' camera block.  Validates and stores only; a camera the library refuses: BhrayError (BHRAY_E_INVALID)."""
        s = still_camera.struct() if still_camera is not None else None
        check(self._L.bhray_accum_set_camera(self._h, C.byref(s) if s is not None else None), self._h, self._L)

    def accum_set_filter(self, filter=None):
        """The reconstruction filter of the accumulation image from the next accum_add on (bhray_accum_set_filter): a StillFilter - .tent(radius),
        .mitchell(radius), .bspline(radius) - or None for the default, the box.  Under a tent or a cubic each sample also feeds the pixels around its own with
        weights that depend on the sample's sub-pixel offset; accum_add_adaptive is then refused (BHRAY_E_STATE).  Validates and stores only; a filter the library
        refuses: BhrayError (BHRAY_E_INVALID)."""
        s = filter.struct() if filter is not None else None
        check(self._L.bhray_accum_set_filter(self._h, C.byref(s) if s is not None else None), self._h, self._L)

    def accum_set_stars(self, on=False):
        """Point stars in the accumulation image from the next accum_add on (bhray_accum_set_stars): with on and a catalogue in force (set_stars),
        every sample image receives the catalogue's stars under the sky pass's footprint rule before it is summed, so the mean holds each star box-filtered at
        sub-pixel accuracy and a filter of accum_set_filter is its point spread function.  Off (the default), or without a catalogue, every image keeps its bits.
        accum_add under a lens and accum_add_adaptive are then refused (BHRAY_E_STATE).  Validates and stores only."""
        check(self._L.bhray_accum_set_stars(self._h, int(on)), self._h, self._L)

    def accum_set_observer(self, velocity=None, beaming=True):
        """The moving observer of the accumulation image from the next accum_add / accum_add_adaptive on (bhray_accum_set_observer): `velocity` is
        beta, the observer's velocity in the static frame, world axes, units of c (|beta| <= 0.99) - or a cameras.Observer, whose own `beaming` then holds.  Every
        generated look direction is Lorentz-aberrated on the device; beaming: every resolved sample is also scaled by the bolometric D^4.  None, or a zero velocity:
        at rest - every image keeps its bits.  Validates and stores only; an observer the library refuses: BhrayError (BHRAY_E_INVALID)."""
        from .cameras import Observer
        if velocity is None:
            check(self._L.bhray_accum_set_observer(self._h, None), self._h, self._L)
            return
        obs = velocity if isinstance(velocity, Observer) else Observer(tuple(float(v) for v in velocity), bool(beaming))
        s = obs.struct()
        check(self._L.bhray_accum_set_observer(self._h, C.byref(s)), self._h, self._L)

    # -- still passes: coverage, geometry, position and escape maps beside the colour (bhray_accum_set_passes)
    def accum_set_passes(self, passes: int = 0):
        """The passes the next accum_begin's accumulation carries beside its colour: an OR of PASS_COVERAGE / PASS_GEOMETRY / PASS_POSITION / PASS_ESCAPE (layouts),
        0 (the default) for none.  Each pass is one more sum plane over the same samples and the same filter; accum_add_adaptive is refused in an accumulation that
        carries one (BHRAY_E_STATE).  Validates and stores only: the running accumulation keeps its set.  Unknown bits: BhrayError (BHRAY_E_INVALID)."""
        check(self._L.bhray_accum_set_passes(self._h, int(passes)), self._h, self._L)

    def accum_passes(self) -> int:
        """The set of the current accumulation (0 before accum_begin)."""
        n = C.c_uint32()
        check(self._L.bhray_accum_passes(self._h, C.byref(n)), self._h, self._L)
        return int(n.value)

    def accum_read_pass(self, pass_bit: int) -> np.ndarray:
        """The mean of one pass over the samples taken so far: (frame_h, frame_w, 4) float32 - (x / w, y / w, z / w, 1), zeros where the pixel took no sample.
        COVERAGE: the horizon, disk and mesh shares; GEOMETRY: closest approach, iterations, transmittance; POSITION: the disk / mesh hit point premultiplied by its
        coverage; ESCAPE: the mean escape direction (its length: the unobstructed share).  Waits.  A pass the accumulation does not carry: BhrayError (BHRAY_E_INVALID)."""
        w, h = int(self.cfg.frame_w), int(self.cfg.frame_h)
        out = np.empty((h, w, 4), dtype=np.float32)
        check(self._L.bhray_accum_read_pass(self._h, int(pass_bit), out.ctypes.data, w * 16), self._h, self._L)
        return out

    # -- adaptive stills: each pixel sampled until the error of its mean is under a bound (bhray_accum_add_adaptive)
    @staticmethod
    def _adaptive_params(min_samples, max_samples, round_samples, tolerance, dark) -> BhrayAccumAdaptive:
        return BhrayAccumAdaptive(C.sizeof(BhrayAccumAdaptive), int(min_samples), int(max_samples), int(round_samples), float(tolerance), float(dark))

    def accum_add_adaptive(self, min_samples: int = 4, max_samples: int = 64, round_samples: int = 4, tolerance: float = 0.05, dark: float = 0.01) -> dict:
        """After accum_begin: min_samples samples for every pixel, then rounds that give the pixels failing the test of include/bhray.h round_samples more, until every
        pixel passes or has max_samples.  Blocks while the rounds run; the reads wait.  Returns {"rounds", "active_last", "rays", "reach"} of this call.  A later call
        (a smaller tolerance, a larger max_samples; the same min_samples and round_samples) continues the accumulation; accum_add does not mix with it."""
        a = self._adaptive_params(min_samples, max_samples, round_samples, tolerance, dark)
        info = BhrayAccumAdaptiveInfo()
        check(self._L.bhray_accum_add_adaptive(self._h, C.byref(a), C.byref(info)), self._h, self._L)
        return info.as_dict()

    def accum_read_counts(self) -> np.ndarray:
        """The number of samples issued to each pixel of an adaptive accumulation: (frame_h, frame_w) uint32.  Waits."""
        w, h = int(self.cfg.frame_w), int(self.cfg.frame_h)
        out = np.empty((h, w), dtype=np.uint32)
        check(self._L.bhray_accum_read_counts(self._h, out.ctypes.data, w * 4), self._h, self._L)
        return out

    def accum_active_pixels(self, min_samples: int = 4, max_samples: int = 64, round_samples: int = 4, tolerance: float = 0.05, dark: float = 0.01) -> np.ndarray:
        """One selection under these parameters without sampling: the indices y * frame_w + x of the pixels that would take more samples, in the order the device
        compacted them (bhray_diag.h)."""
        a = self._adaptive_params(min_samples, max_samples, round_samples, tolerance, dark)
        out = np.empty(int(self.cfg.frame_w) * int(self.cfg.frame_h), dtype=np.uint32)
        n = C.c_uint32()
        check(self._L.bhray_accum_active_pixels(self._h, C.byref(a), out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)), self._h, self._L)
        return out[:int(n.value)].copy()

    # -- per frame
    def set_uniforms(self, camera: bytes, black_hole: bytes, details: bytes):
        assert len(camera) == 32 and len(black_hole) == 132 and len(details) == 32
        check(self._L.bhray_set_uniforms(self._h, camera, black_hole, details), self._h, self._L)

    def render(self):
        check(self._L.bhray_render(self._h), self._h, self._L)

    def flush(self):
        """frames_per_batch > 1: enqueue the launches of the frames staged so far."""
        check(self._L.bhray_flush(self._h), self._h, self._L)

    def sync(self):
        check(self._L.bhray_sync(self._h), self._h, self._L)

    # -- output
    @property
    def frame_size(self):
        return int(self.cfg.frame_w), int(self.cfg.frame_h)

    def local_rows(self) -> np.ndarray:
        n = int(self._L.bhray_local_rows(self._h))
        out = np.zeros(n, dtype=np.uint32)
        r = C.c_uint32()
        for i in range(n):
            check(self._L.bhray_local_row_index(self._h, i, C.byref(r)), self._h, self._L)
            out[i] = r.value
        return out

    def read_hdr(self) -> np.ndarray:
        n = int(self._L.bhray_local_rows(self._h))
        out = np.empty((n, int(self.cfg.frame_w), 4), dtype=np.float32)
        check(self._L.bhray_read_hdr(self._h, out.ctypes.data, int(self.cfg.frame_w) * 16), self._h, self._L)
        return out

    def read_hdr_async(self, dst: "PinnedFrame") -> int:
        """Enqueue the device->host copy of the most recently enqueued frame into pinned memory, behind its kernels; returns a ticket."""
        t = C.c_uint64()
        check(self._L.bhray_read_hdr_async(self._h, C.c_void_p(dst.ptr), int(self.cfg.frame_w) * 16, C.byref(t)), self._h, self._L)
        return int(t.value)

    def read_sky_async(self, dst: "PinnedFrame") -> int:
        """The RGBA16F image of the sky pass (resolve_sky first) into pinned memory (a PinnedFrame(rows, width, channels16=True))."""
        t = C.c_uint64()
        check(self._L.bhray_read_sky_async(self._h, C.c_void_p(dst.ptr), int(self.cfg.frame_w) * 8, C.byref(t)), self._h, self._L)
        return int(t.value)

    def wait_read(self, ticket: int):
        check(self._L.bhray_wait_read(self._h, C.c_uint64(ticket)), self._h, self._L)

    def import_external_fd(self, fd: int, nbytes: int) -> int:
        """Map memory exported by another API (Vulkan OPAQUE_FD / dma-buf) on the GPU that delivers the frame; returns a device pointer for bind_output."""
        p = C.c_void_p()
        check(self._L.bhray_import_external_fd(self._h, int(fd), nbytes, C.byref(p)), self._h, self._L)
        return p.value

    def release_external(self, ptr: int):
        check(self._L.bhray_release_external(self._h, C.c_void_p(ptr)), self._h, self._L)

    def read_level(self, level: int) -> np.ndarray:
        w, h = int(self.cfg.level_w[level]), int(self.cfg.level_h[level])
        out = np.empty((h, w, 4), dtype=np.float32)
        check(self._L.bhray_read_level(self._h, level, out.ctypes.data, out.strides[0]), self._h, self._L)
        return out

    def resolve_sky(self):
        """sky.wgsl behind the last frame (mod.rs:419): direction pixels -> sky^4; RGBA16F."""
        check(self._L.bhray_resolve_sky(self._h), self._h, self._L)

    def read_sky(self) -> np.ndarray:
        n = int(self._L.bhray_local_rows(self._h))
        out = np.empty((n, int(self.cfg.frame_w), 4), dtype=np.float16)
        check(self._L.bhray_read_sky(self._h, out.ctypes.data, int(self.cfg.frame_w) * 8), self._h, self._L)
        return out

    # -- footprint-filtered sky pass
    def set_sky_filter(self, mode):
        """0 / False: the sky pass is sky.wgsl (the default).  1 / True: from the next resolve_sky (and the sky pass resolve_display runs) every direction pixel whose
        footprint - the difference to its neighbours' directions - exceeds one sky texel takes 1 to 8 taps from a mip pyramid of the sky texture.  Waits for the
        frames in flight and builds the pyramid.  BhrayError (BHRAY_E_STATE) on a ctx that splits the frame; trace_rays(sky=True) and accum_* are not affected."""
        check(self._L.bhray_set_sky_filter(self._h, int(mode)), self._h, self._L)

    def read_sky_pyramid_level(self, level: int, size) -> np.ndarray:
        """Level `level` >= 1 of the sky pyramid, (h, w, 4) float16; size = (w, h) of that level (sky_pyramid_sizes).  Needs the filter on (bhray_diag.h)."""
        w, h = int(size[0]), int(size[1])
        out = np.empty((h, w, 4), dtype=np.float16)
        check(self._L.bhray_read_sky_pyramid_level(self._h, int(level), out.ctypes.data, w * h), self._h, self._L)
        return out

    # -- point stars
    def set_stars(self, stars, params=None):
        """A star catalogue lensed into the sky pass: from the next resolve_sky (and the sky pass resolve_display runs) every direction pixel whose footprint is known
        receives the flux of the catalogue stars inside it over the footprint's solid angle.  stars: None (or an empty array) removes the catalogue; otherwise an
        (n, 6) float32 array of (dir x y z, flux r g b) rows, or an array of layouts.BhrayStar.  params: a layouts.BhrayStarParams, or None for the defaults.  Waits
        for the frames in flight.  BhrayError (BHRAY_E_STATE) on a ctx that splits the frame; read_hdr, trace_rays(sky=True) and accum_* are not affected."""
        a, n = star_array(stars)
        p = C.byref(params) if params is not None else None
        check(self._L.bhray_set_stars(self._h, a.ctypes.data if n else None, n, p), self._h, self._L)

    def star_image(self, frame, sky_in=None) -> np.ndarray:
        """The star kernel with this ctx's catalogue over a supplied (h, w, 4) float32 frame (bhray_diag_star_image): (h, w, 4) float16, the stars added to sky_in
        (None: zeros)."""
        f = np.ascontiguousarray(frame, dtype=np.float32)
        if f.ndim != 3 or f.shape[2] != 4:
            raise ValueError("star_image takes an (H, W, 4) float32 frame")
        h, w = f.shape[:2]
        s = None
        if sky_in is not None:
            s = np.ascontiguousarray(sky_in)
            if s.dtype not in (np.float16, np.uint16) or s.shape != f.shape:
                raise ValueError("sky_in is an (H, W, 4) binary16 image of the frame's size")
        out = np.empty((h, w, 4), dtype=np.float16)
        check(self._L.bhray_diag_star_image(self._h, f.ctypes.data, w, h, s.ctypes.data if s is not None else None, out.ctypes.data), self._h, self._L)
        return out

    # -- display pass: bloom, mix, ACES, FXAA into the RGBA8 sRGB image
    def set_post_uniforms(self, fxaa: BhrayFxaaDetails | bytes | None = None, mix: BhrayMixDetails | bytes | float | None = None):
        """The FXAA (16 B) and mix (4 B) uniform blocks, applied from the next resolve_display; None = the reference's defaults."""
        df, dm = post_defaults()
        f = bytes(fxaa) if fxaa is not None else bytes(df)
        m = bytes(BhrayMixDetails(float(mix))) if isinstance(mix, (int, float)) else (bytes(mix) if mix is not None else bytes(dm))
        assert len(f) == 16 and len(m) == 4
        check(self._L.bhray_set_post_uniforms(self._h, f, m), self._h, self._L)

    def resolve_display(self):
        """The display pass behind the last frame (runs the sky pass first if it has not run for that frame)."""
        check(self._L.bhray_resolve_display(self._h), self._h, self._L)

    def read_display(self) -> np.ndarray:
        """uint8 [H, W, 4]: R, G, B sRGB-encoded, A unorm.  On a rank that does not hold the frame (a non-root rank of a one-process-per-GPU
        ctx: bhray_local_rows is 0) the library delivers nothing and this returns a [0, W, 4] array."""
        w = int(self.cfg.frame_w)
        h = int(self.cfg.frame_h) if int(self._L.bhray_local_rows(self._h)) > 0 else 0
        out = np.empty((h, w, 4), dtype=np.uint8)
        check(self._L.bhray_read_display(self._h, out.ctypes.data if h else None, w * 4), self._h, self._L)
        return out

    def read_display_async(self, dst: "PinnedFrame") -> int:
        """The RGBA8 image (resolve_display first) into pinned memory (a PinnedFrame(rows, width, rgba8=True)); returns a ticket."""
        t = C.c_uint64()
        check(self._L.bhray_read_display_async(self._h, C.c_void_p(dst.ptr), int(self.cfg.frame_w) * 4, C.byref(t)), self._h, self._L)
        return int(t.value)

    def display_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._L.bhray_display_device_ptr(self._h, C.byref(p), C.byref(n)), self._h, self._L)
        return p.value, n.value

    def device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._L.bhray_hdr_device_ptr(self._h, C.byref(p), C.byref(n)), self._h, self._L)
        return p.value, n.value

    def bind_output(self, ptr, nbytes):
        check(self._L.bhray_bind_output(self._h, C.c_void_p(ptr), nbytes), self._h, self._L)

    def wait_stream(self, s):
        """The next render starts after everything enqueued so far on hipStream_t `s`."""
        check(self._L.bhray_wait_stream(self._h, C.c_void_p(s)), self._h, self._L)

    def next_stream(self) -> int:
        """hipStream_t (as int) of the slot the next render will use."""
        s = C.c_void_p()
        check(self._L.bhray_next_stream(self._h, C.byref(s)), self._h, self._L)
        return s.value

    def signal_stream(self, s):
        """Work enqueued on hipStream_t `s` from now on starts after the last render."""
        check(self._L.bhray_signal_stream(self._h, C.c_void_p(s)), self._h, self._L)

    def counters(self) -> dict:
        c = BhrayCounters()
        check(self._L.bhray_get_counters(self._h, C.byref(c)), self._h, self._L)
        return c.as_dict()

    def scheduling_counters(self) -> dict:
        """wave steps, rays adopted through the drain-merging mailbox, lane occupancy of the step loop (needs counters=True)"""
        c = BhrayCounters()
        check(self._L.bhray_get_counters(self._h, C.byref(c)), self._h, self._L)
        return c.scheduling()

    def level_counters(self, level: int) -> dict:
        c = BhrayCounters()
        check(self._L.bhray_get_level_counters(self._h, level, C.byref(c)), self._h, self._L)
        return c.as_dict()

    def selftest(self):
        """(1/x mismatches, sqrt mismatches, places where the portable acos increases): exhaustive device checks of the
        properties the exact shortcuts rest on; all must be 0."""
        m = (C.c_uint64 * 3)()
        check(self._L.bhray_selftest(self._h, m), self._h, self._L)
        return int(m[0]), int(m[1]), int(m[2])

    def trace_builds(self):
        """(trace launches enqueued so far with an ORIGIN build - the hole at +0, +0, +0 in every frame of the batch -, with any other build): bhray_get_trace_builds"""
        m = (C.c_uint64 * 2)()
        check(self._L.bhray_get_trace_builds(self._h, m), self._h, self._L)
        return int(m[0]), int(m[1])

    def level_grids(self, slot: int = 0) -> dict:
        """Trace grids sized by queue length (bhray_get_level_grids): for the batch frame slot `slot` launched last, the blocks each ladder trace launch got and the
        rays it was sized from (None: not sized - it got `ctx_grid`); and the ctx's totals of ladder trace launches, their blocks, and launches at the ceiling."""
        from .layouts import BhrayLevelGridInfo
        g = BhrayLevelGridInfo()
        check(self._L.bhray_get_level_grids(self._h, slot, C.byref(g)), self._h, self._L)
        return g.as_dict()

    def err_skip(self):
        """(RK wave-steps of the last render, those whose active lanes all satisfied the error-estimate bound, lane-steps that satisfied it with an estimate above the
        step-size threshold - must be 0): bhray_get_err_skip (needs counters=True)"""
        m = (C.c_uint64 * 3)()
        check(self._L.bhray_get_err_skip(self._h, m), self._h, self._L)
        return int(m[0]), int(m[1]), int(m[2])

    def timing(self) -> BhrayTiming:
        t = BhrayTiming()
        check(self._L.bhray_get_timing(self._h, C.byref(t)), self._h, self._L)
        return t


class PinnedFrame:
    """Pinned host memory for one RGBA32F frame (bhray_host_alloc), viewed as a (rows, width, 4) float32 array
    (channels16: RGBA16F, float16; rgba8: the display image, uint8)."""

    def __init__(self, rows: int, width: int, channels16: bool = False, rgba8: bool = False):
        assert not (channels16 and rgba8)
        p = C.c_void_p()
        self.nbytes = rows * width * (4 if rgba8 else (8 if channels16 else 16))
        check(lib().bhray_host_alloc(self.nbytes, C.byref(p)))
        self.ptr = p.value
        if rgba8:               # RGBA8 sRGB (the display pass's image)
            self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(rows, width, 4))
        elif channels16:        # RGBA16F (the sky pass's image)
            self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint16)), shape=(rows, width, 4)).view(np.float16)
        else:
            self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(rows, width, 4))

    def free(self):
        p, self.ptr = self.ptr, None
        if p:
            self.array = None
            check(lib().bhray_host_free(C.c_void_p(p)))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Renderer:
    """Renderer::{new,render} restricted to the ray pass (mod.rs:113-207, 378-420)."""

    def __init__(self, cfg: BhrayConfig | None = None, device=0, **kw):
        self.camera = Camera()
        self.black_hole = BlackHole()
        self.ray_details = RayDetails()                      # mod.rs:116-121
        self.ray_pass = RayPass(cfg if cfg is not None else ladder_from_base((72, 41), 3, 4), device=device, **kw)
        self.models: list[Model] = []                        # scene.models: slot i of the ctx holds models[i]
        self._device_built: list[bool] = []                  # ... and whether its tree was built on the GPU (add_model(build="device"))
        self.mesh_lensing = False                            # lensed meshes (RayPass.set_mesh_lensing): applied before each render
        self.lens_ray_batches = False                        # ... and, with it, ray batches too (LENS_RAYS): render_rays, render_records, pick, the stills
        self._lensing_applied = 0                            # the word the ctx was last told (its default: off)
        self.still_info = None                               # what the last adaptive still did (render_still(adaptive=...)): rounds, active_last, rays, reach
        self.sky_filter = False                              # footprint-filtered sky pass (RayPass.set_sky_filter): applied before save_image's display pass
        self._sky_filter_applied = False
        self.stars = None                                    # the point-star catalogue in force (set_stars): an (n, 6) float32 array, or None

    def set_stars(self, stars, params=None):
        """A star catalogue lensed into the sky pass (RayPass.set_stars): in force from the next resolve_sky / save_image on; None removes it.  A refused
        call leaves Renderer.stars, like the ctx's catalogue, as it was."""
        self.ray_pass.set_stars(stars, params)
        a, n = star_array(stars)
        self.stars = a.copy() if n else None

    @property
    def model(self) -> Model | None:
        return self.models[0] if self.models else None

    def set_model(self, model: Model):
        """Model slot 0 (replaced if it is there)."""
        self.ray_pass.upload_model(model, 0)
        if self.models:
            self.models[0], self._device_built[0] = model, False
        else:
            self.models.append(model); self._device_built.append(False)
        self.ray_details.model_count = len(self.models)      # mod.rs:384 (scene.models.size())

    def add_model(self, model: Model, build: str = "host") -> int:
        """One more model in the next slot (up to MAX_MODELS); returns its index, the model_index of RayPass.set_model_transform.
        build="device": the tree is built on the GPU (RayPass.upload_model_build) and the model's own tree is not read."""
        index = len(self.models)
        if index >= MAX_MODELS:
            raise ValueError(f"add_model: the ctx holds {MAX_MODELS} models")
        if build not in ("host", "device"):
            raise ValueError(f"add_model: build must be 'host' or 'device', got {build!r}")
        if build == "device":
            self.ray_pass.upload_model_build(model, index)
        else:
            self.ray_pass.upload_model(model, index)
        self.models.append(model); self._device_built.append(build == "device")
        self.ray_details.model_count = len(self.models)      # mod.rs:384 (scene.models.size())
        return index

    def set_model_rotation(self, index: int, rotation, pivot=(0.0, 0.0, 0.0), scale: float = 1.0):
        """What the reference's Model.rotation promises and never does: model `index` (added with build="device") turned by the Euler angles `rotation`
        about `pivot` (model space), scaled by `scale` - on the GPU, from its rest geometry (pose_from_euler + RayPass.set_model_pose)."""
        if not 0 <= index < len(self.models):
            raise ValueError(f"set_model_rotation: no model {index}")
        if not self._device_built[index]:
            raise ValueError(f"set_model_rotation: model {index} was built on the host; add it with build='device'")
        self.ray_pass.set_model_pose(pose_from_euler(rotation, pivot, scale), index)

    def render(self, dt: float = 0.0):
        self.ray_details.time += dt                          # mod.rs:382
        self.ray_pass.set_uniforms(self.camera.uniform(), self.black_hole.uniform(), self.ray_details.uniform())
        self._apply_lensing()
        self.ray_pass.render()

    def read_hdr(self):
        return self.ray_pass.read_hdr()

    def render_rays(self, rays, shape, resolve_sky: bool = False):
        """An image seen through caller-supplied rays (bhusie_amd.cameras: pinhole_rays, equirect_rays, fisheye_rays, or any (h * w, 6 | 8) array) under this
        renderer's black hole, details, textures and models: (h, w, 4) float32 - (colour, 1) or (escape direction, 0), as read_hdr.  A ray with a zero
        direction or a non-finite component (a fisheye's pixels outside its circle) is not traced: (0, 0, 0, -1).  resolve_sky=True: the RGBA16F image of the
        sky pass over it instead (RayPass.resolve_sky's semantics; the untraced pixels pass through: black, alpha -1)."""
        h, w = int(shape[0]), int(shape[1])
        rec = RayPass._ray_records(rays)
        if rec.shape[0] != h * w:
            raise ValueError(f"render_rays: {rec.shape[0]} rays for a {w}x{h} image")
        self.ray_pass.set_uniforms(self.camera.uniform(), self.black_hole.uniform(), self.ray_details.uniform())
        self._apply_lensing()
        six = rec[:, [0, 1, 2, 4, 5, 6]]
        usable = np.isfinite(six).all(axis=1) & (rec[:, 4:7] != 0.0).any(axis=1)
        img = np.zeros((h * w, 4), dtype=np.float16 if resolve_sky else np.float32)
        img[:, 3] = -1.0
        if usable.any():
            got = self.ray_pass.trace_rays(rec[usable], sky=resolve_sky)
            img[usable] = got[1] if resolve_sky else got
        return img.reshape(h, w, 4)

    def _lensing_word(self) -> int:
        """what the ctx is to be told: LENS_FRAMES | LENS_RAYS, LENS_FRAMES, or 0"""
        if not self.mesh_lensing:
            return 0
        return (LENS_FRAMES | LENS_RAYS) if self.lens_ray_batches else LENS_FRAMES

    def _apply_lensing(self):
        word = self._lensing_word()
        if word != self._lensing_applied:                    # the value last sent, not its truth: 1 and 3 are different settings
            self.ray_pass.set_mesh_lensing(word)
            self._lensing_applied = word

    def _apply_uniforms(self):
        self.ray_pass.set_uniforms(self.camera.uniform(), self.black_hole.uniform(), self.ray_details.uniform())
        self._apply_lensing()

    def render_records(self, rays, shape):
        """The record layers of an image seen through caller-supplied rays (render_rays' rays and rules): an (h, w) structured array (RAY_RECORD_DTYPE) -
        position, hit, triangle, iterations, closest, transmittance per pixel.  A ray that is not traced (zero direction, non-finite component):
        hit = HIT_UNUSABLE, triangle = -1, everything else zero, as the device form answers it."""
        h, w = int(shape[0]), int(shape[1])
        rec = RayPass._ray_records(rays)
        if rec.shape[0] != h * w:
            raise ValueError(f"render_records: {rec.shape[0]} rays for a {w}x{h} image")
        self._apply_uniforms()
        six = rec[:, [0, 1, 2, 4, 5, 6]]
        usable = np.isfinite(six).all(axis=1) & (rec[:, 4:7] != 0.0).any(axis=1)
        layers = np.zeros(h * w, dtype=RAY_RECORD_DTYPE)
        layers["hit"] = HIT_UNUSABLE
        layers["triangle"] = -1
        if usable.any():
            layers[usable] = self.ray_pass.trace_rays_records(rec[usable])[1]
        return layers.reshape(h, w)

    def pick(self, x: int, y: int) -> dict:
        """What is under frame pixel (x, y)?  Traces that pixel's pinhole ray (cameras.pinhole_rays' arithmetic for the one pixel: create_ray at the frame's
        size) under the renderer's current scene and returns its record: {hit (HIT_*), model (the slot of a HIT_MESH hit, else None), triangle (index into
        that model's triangles, else -1), position, iterations, closest, transmittance}."""
        fw, fh = int(self.ray_pass.cfg.frame_w), int(self.ray_pass.cfg.frame_h)
        if not (0 <= int(x) < fw and 0 <= int(y) < fh):
            raise ValueError(f"pick: pixel ({x}, {y}) lies outside the {fw}x{fh} frame")
        self._apply_uniforms()
        r = self.ray_pass.trace_rays_records(pinhole_rays(self.camera, fw, fh, pixel=(int(x), int(y))))[1][0]
        kind = int(r["hit"]) & 0xFF
        return {"hit": kind, "model": (int(r["hit"]) >> 8) & 0xFF if kind == HIT_MESH else None, "triangle": int(r["triangle"]),
                "position": tuple(float(v) for v in r["position"]), "iterations": int(r["iterations"]),
                "closest": float(r["closest"]), "transmittance": float(r["transmittance"])}

    def ray_path(self, x: int, y: int, stride_log2: int = 0) -> dict:
        """The light path behind frame pixel (x, y): pick's dictionary, and `path` - a (k, 3) float32 array, the points of that pixel's pinhole ray from the camera to where
        trace_ray's loop ended, one per 2**stride_log2 iterations and the end point - and `path_iterations`, (k,) uint32: the iteration each point belongs to.  The row
        is sized from max_iterations, so nothing is dropped."""
        fw, fh = int(self.ray_pass.cfg.frame_w), int(self.ray_pass.cfg.frame_h)
        if not (0 <= int(x) < fw and 0 <= int(y) < fh):
            raise ValueError(f"ray_path: pixel ({x}, {y}) lies outside the {fw}x{fh} frame")
        self._apply_uniforms()
        max_points = (int(self.ray_details.max_iterations) >> int(stride_log2)) + 2
        _, rec, pts, cnt = self.ray_pass.trace_rays_paths(pinhole_rays(self.camera, fw, fh, pixel=(int(x), int(y))), stride_log2, max_points)
        r, k = rec[0], int(cnt[0])
        assert k <= max_points
        kind = int(r["hit"]) & 0xFF
        return {"hit": kind, "model": (int(r["hit"]) >> 8) & 0xFF if kind == HIT_MESH else None, "triangle": int(r["triangle"]),
                "position": tuple(float(v) for v in r["position"]), "iterations": int(r["iterations"]),
                "closest": float(r["closest"]), "transmittance": float(r["transmittance"]),
                "path": pts["position"][0, :k].copy(), "path_iterations": pts["iteration"][0, :k].copy()}

    def _accumulate(self, samples: int, shutter: float, camera=None, filter=None, stars=False, observer=None, passes=0):
        samples = int(samples)
        if samples < 1:
            raise ValueError(f"render_still: samples must be at least 1, got {samples}")
        self._apply_uniforms()
        self.ray_pass.accum_set_camera(camera)
        self.ray_pass.accum_set_filter(filter)
        self.ray_pass.accum_set_stars(bool(stars))
        self.ray_pass.accum_set_observer(observer)
        self.ray_pass.accum_set_passes(self._pass_bits(passes))
        self.ray_pass.accum_begin()
        if not shutter > 0.0:
            self.ray_pass.accum_add(samples)
            return
        t0 = self.ray_details.time
        try:
            for s in range(samples):                         # one sample per call: each under its own `time`
                self.ray_details.time = t0 + float(shutter) * s / samples
                self._apply_uniforms()
                self.ray_pass.accum_add(1)
        finally:
            self.ray_details.time = t0

    @staticmethod
    def _pass_bits(passes) -> int:
        """an OR of PASS_* bits from an int, a pass name, or an iterable of names and bits"""
        if passes is None:
            return 0
        if isinstance(passes, str):
            passes = [p for p in passes.split(",") if p]
        if isinstance(passes, (int, np.integer)):
            return int(passes)
        bits = 0
        for p in passes:
            if isinstance(p, str):
                if p not in PASS_NAMES:
                    raise ValueError(f"unknown still pass {p!r}: one of {', '.join(PASS_NAMES)}")
                bits |= PASS_NAMES[p]
            else:
                bits |= int(p)
        return bits

    def still_pass(self, name_or_bit) -> np.ndarray:
        """One pass of the last still rendered with `passes` (RayPass.accum_read_pass): "coverage", "geometry", "position", "escape" or the PASS_*
        bit - (frame_h, frame_w, 4) float32, the mean over the still's samples under its filter.  A pass the still does not carry: BhrayError (BHRAY_E_INVALID)."""
        bit = self._pass_bits(name_or_bit)
        return self.ray_pass.accum_read_pass(bit)

    def render_still(self, samples: int = 16, shutter: float = 0.0, adaptive: AdaptiveStill | None = None, camera=None, filter=None, stars: bool = False,
                     observer=None, passes=0, denoise=None) -> np.ndarray:
        """A supersampled still of the current scene (RayPass.accum_*): the mean of `samples` jittered samples per frame pixel, sky resolved,
        (frame_h, frame_w, 4) float32.  Sample 0 is the pixel centre, so samples=1 is the frame a `levels = 1` ladder renders, after the sky pass in binary32.
        shutter > 0: motion blur - sample s is rendered at ray_details.time + shutter * s / samples (the disk turns with `time`); ray_details.time is left as it was.
        adaptive: an AdaptiveStill - each pixel is sampled until the error of its mean is under the bound; `samples` is then not read, the motion blur is
        not available (ValueError), still_info holds what the call did and still_counts() delivers the per-pixel sample counts.
        camera: a cameras.StillCamera - the still as a 360 x 180 degree panorama (.equirect()), a fisheye (.fisheye(fov)) or through a thin lens
        (.pinhole(lens_radius, focus_distance): depth of field; sample 0 is then a lens sample, not the centre ray) from the scene camera's position along its forward
        (DESIGN.md §21); None: the pinhole.  The ctx keeps the camera of the last still.
        filter: a StillFilter - the pixel reconstruction filter, StillFilter.tent(radius), .mitchell(radius) or .bspline(radius); None: the box.  Not
        with `adaptive` (ValueError).  The ctx keeps the filter of the last still.
        stars: the catalogue of set_stars lensed into every sample's image: pixel-sharp stars at sub-pixel accuracy, with `filter` as their point
        spread function.  Without a catalogue it changes nothing.  Not with `adaptive` (ValueError) or a camera with a lens (BhrayError).  The ctx keeps the
        switch of the last still.
        observer: a cameras.Observer - the still as a moving observer sees it: Observer((vx, vy, vz)) aberrates every look direction by the
        velocity (static frame, world axes, units of c), and with beaming (the default) scales every sample by D^4; goes with `adaptive`, every camera, the filters and
        the stars.  None: at rest.  The ctx keeps the observer of the last still.
        passes: the per-pixel maps the still carries beside its colour - an OR of PASS_COVERAGE / PASS_GEOMETRY / PASS_POSITION / PASS_ESCAPE, or
        their names ("coverage,escape", ["geometry"]); still_pass(name) then delivers each.  The colour keeps its bits.  Not with `adaptive` (ValueError).  0: none.
        denoise: a StillDenoise, or True for the library's defaults - the still is delivered through the a-trous filter guided by its passes; with
        passes == 0 all four passes are switched on.  None or False: the plain mean.  Not with `adaptive` (ValueError)."""
        if denoise is False:
            denoise = None
        if denoise is not None and adaptive is not None:
            raise ValueError("render_still: an adaptive still is not denoised (it carries no passes)")
        if adaptive is None:
            if denoise is not None and self._pass_bits(passes) == 0:
                passes = PASS_ALL
            self._accumulate(samples, shutter, camera, filter, stars, observer, passes)
            return self.ray_pass.accum_read() if denoise is None else self.ray_pass.accum_read_denoised(denoise)
        if self._pass_bits(passes):
            raise ValueError("render_still: an adaptive still carries no passes (its adder works over a pixel list)")
        if stars:
            raise ValueError("render_still: an adaptive still has no point stars (a round's pixels take different samples)")
        if filter is not None and filter.kind != FILTER_BOX:
            raise ValueError("render_still: an adaptive still has no filter but the box (a round's pixels take different samples)")
        if shutter > 0.0:
            raise ValueError("render_still: an adaptive still has no shutter (every pixel takes its own number of samples)")
        self._apply_uniforms()
        self.ray_pass.accum_set_camera(camera)
        self.ray_pass.accum_set_filter(None)
        self.ray_pass.accum_set_stars(False)
        self.ray_pass.accum_set_observer(observer)
        self.ray_pass.accum_set_passes(0)
        self.ray_pass.accum_begin()
        self.still_info = self.ray_pass.accum_add_adaptive(**adaptive.as_kwargs())
        return self.ray_pass.accum_read()

    def still_counts(self) -> np.ndarray:
        """The sample-count heat map of the last adaptive still: (frame_h, frame_w) uint32."""
        return self.ray_pass.accum_read_counts()

    def save_still(self, path, samples: int = 16, camera=None, filter=None, stars: bool = False, observer=None, passes=0, denoise=None):
        """save_image for a supersampled still: the mean of `samples` samples per pixel through the display pass, written with alpha 255.  camera, filter, stars,
        observer, passes, denoise: as render_still's (still_pass delivers the passes afterwards)."""
        from PIL import Image
        if denoise is False:
            denoise = None
        if denoise is not None and self._pass_bits(passes) == 0:
            passes = PASS_ALL
        self._accumulate(samples, 0.0, camera, filter, stars, observer, passes)
        img = self.ray_pass.accum_read_display() if denoise is None else self.ray_pass.accum_read_display_denoised(denoise)
        img[..., 3] = 255
        Image.fromarray(img, "RGBA").save(path)

    def save_image(self, path):
        """The reference's Save Image (mod.rs:473-482): the display pass's RGBA8 image of the last frame, written with alpha 255
        (PIL picks the format from the file name; PNG as the reference does)."""
        from PIL import Image
        if bool(self.sky_filter) != self._sky_filter_applied:
            self.ray_pass.set_sky_filter(bool(self.sky_filter))
            self._sky_filter_applied = bool(self.sky_filter)
            self.ray_pass.resolve_sky()                      # a sky image this frame already has was made under the other mode
        self.ray_pass.resolve_display()
        img = self.ray_pass.read_display()
        img[..., 3] = 255
        Image.fromarray(img, "RGBA").save(path)
