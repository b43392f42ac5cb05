"""-m gpu: the trace wave's phases (refill, disk shading, flat passes, epilogue) and the hit tests on the step's rare path with the short correctly rounded
sequences of N8 (bhray_kernels.hip, BHRAY_PHASE_SEQ: rcp_rn / sqrt_rn, the `_ph` twins, dist_rsqrt_rn, two_over_rn, and unorm8_rn for a texel's byte / 255) against the
kernels before them - the same sources built with -DBHRAY_PHASE_SEQ=0 (`make -C bhusie_amd/csrc phases0` -> libbhray_phases0.so, built by __graft_entry__.build();
test infrastructure: the compiler's IEEE lowering everywhere, the parent's trace kernels instruction for instruction).  Every sequence returns the IEEE result on
every input, so every frame must be the same BYTES whichever library rendered it - colour pixels, direction pixels and classes alike (the optical depth's
pow(x, 1.3) is the device library's in both) - and a counting ctx must count the same.  One exception, DESIGN.md §2's: the SIGN of a NaN that both frames hold in the
same word is not specified and differs between builds of the same source - measured here: the camera outside the sphere with the hole off the origin has one colour
pixel of 160x90 (row 49, column 98) whose optical depth is the power of a negative density, 0xffc00000 from the shipped dense RK build and 0x7fc00000 from phases0's, in
all three channels; a NaN against a number, a NaN's payload and every other bit count.  Ladders of three levels to 96x54 and 160x90.  The dense builds are forced
with BHRAY_TRACE_DENSE=1 (read at create) on 22 frame slots; one frame slot runs the latency builds, whose coarse levels are thin shares and quad launches."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T

pytestmark = pytest.mark.gpu

OFF = (0.5, -0.25, 1.0)
OUTSIDE = dict(position=(0.0, 3.0, -45.0), forward=(0.0, -3.0 / 45.1, 45.0 / 45.1), fov=1.0)      # a camera outside the relativity sphere: the flat phase from the first iteration
LADDERS = [((96, 54), 3, 3), ((160, 90), 3, 3)]                                                   # frame, multiplier, levels


@pytest.fixture
def phases0_library():
    from bhusie_amd import _lib, layouts
    path = T.variant_library("phases0")
    saved = _lib.lib()
    L = C.CDLL(path)
    layouts.declare(L)

    def use(phases0: bool):
        _lib._lib = L if phases0 else saved
    yield use
    _lib._lib = saved


def both(phases0_library, fn):
    phases0_library(False); a = fn()
    phases0_library(True); b = fn()
    phases0_library(False)
    return a, b


def same_bytes(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape
        nan_both = np.isnan(x) & np.isnan(y)                       # the sign of a NaN both frames hold is unspecified; its payload is compared
        clear = np.where(nan_both, np.uint32(0x7fffffff), np.uint32(0xffffffff))
        d = (x.view(np.uint32) & clear) != (y.view(np.uint32) & clear)
        where = np.argwhere(d.any(axis=-1))[:3]
        assert not d.any(), (f"{what}, case {i}: {int(d.any(axis=-1).sum())} pixels differ between the shipped library and phases0, first at {where.tolist()}: "
                             f"{[(x[r, c].tolist(), [hex(v) for v in x[r, c].view(np.uint32)], y[r, c].tolist(), [hex(v) for v in y[r, c].view(np.uint32)]) for r, c in where]}")
        assert (x[..., 3] == 1.0).any() and (x[..., 3] == 0.0).any(), f"{what}, case {i}: the frame has no colour pixel or no direction pixel - the case tests nothing"


def scenes(method, **extra):
    """hole at the origin and off it, camera outside the sphere, disk texture / red shift on and off, step size 1 (horizon hits within a step)"""
    u = lambda **kw: T.uniforms(integration_method=method, **extra, **kw)
    return [u(),
            u(black_hole=B.BlackHole(position=OFF)),
            u(camera=B.Camera(**OUTSIDE)),
            u(camera=B.Camera(**OUTSIDE), black_hole=B.BlackHole(position=OFF)),
            u(black_hole=B.BlackHole(show_disk_texture=0, show_red_shift=1)),
            u(black_hole=B.BlackHole(show_disk_texture=1, show_red_shift=0, position=OFF)),
            u(black_hole=B.BlackHole(show_disk_texture=0, show_red_shift=0)),
            u(step_size=1.0),
            u(step_size=1.0, black_hole=B.BlackHole(position=OFF))]


def frames_of(cases, tex, model=None, frames=1):
    out = []
    for cfg, u, kw in cases:
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        if model is not None:
            rp.upload_model(model)
        rp.set_uniforms(*u)
        for _ in range(frames):
            rp.render()
        rp.sync()
        out.append(rp.read_hdr().copy())
        rp.close()
    return out


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("spec", [0, 2])
def test_one_frame_slot_latency_builds_thin_and_quad_launches(phases0_library, method, spec):
    tex = T.textures()
    cases = [(B.ladder_for_frame(*shape), u, dict(frames_in_flight=1, speculative_levels=spec)) for shape in LADDERS for u in scenes(method)]
    a, b = both(phases0_library, lambda: frames_of(cases, tex))
    same_bytes(a, b, f"one slot, method {method}, speculative levels {spec}")


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("spec", [0, 2])
def test_22_frame_slots_dense_builds(phases0_library, monkeypatch, method, spec):
    monkeypatch.setenv("BHRAY_TRACE_DENSE", "1")
    tex = T.textures()
    cases = [(B.ladder_for_frame(*shape), u, dict(frames_in_flight=22, speculative_levels=spec)) for shape in LADDERS for u in scenes(method)]
    a, b = both(phases0_library, lambda: frames_of(cases, tex, frames=3))
    same_bytes(a, b, f"22 slots, dense builds, method {method}, speculative levels {spec}")


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("dense", [0, 1])
def test_small_mesh_rare_path_and_bvh_flat_phase(phases0_library, monkeypatch, tmp_path, method, dense):
    """The mesh variant.  dense 1: the dense mesh build has the sequences - the mesh case of this change (rare path plus BVH flat phase).  dense 0: the latency mesh builds
    keep the IEEE forms (BHRAY_PHASE_SEQ's bit 3 is off), so both libraries run the same text there: a guard for the day the bit is set, not coverage of this change."""
    from bhusie_amd import assets
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    p = tmp_path / "mesh.obj"
    p.write_text(assets.icosphere_mesh_obj(2, radius=6.0, bump=0.2, seed=11))
    model = B.load_model(str(p))
    model.set_transform((-7.0, 1.0, 24.0), 1)
    kw = dict(frames_in_flight=22 if dense else 1, speculative_levels=0)
    cases = [(B.ladder_for_frame(*shape), u, kw) for shape in LADDERS
             for u in (T.uniforms(integration_method=method, model_count=1), T.uniforms(integration_method=method, model_count=1, camera=B.Camera(**OUTSIDE)),
                       T.uniforms(integration_method=method, model_count=1, black_hole=B.BlackHole(position=OFF)))]
    a, b = both(phases0_library, lambda: frames_of(cases, tex, model=model))
    same_bytes(a, b, f"mesh, method {method}, dense {dense}")


@pytest.mark.parametrize("method", [0, 1])
def test_counting_ctx_same_bytes_and_equal_counters(phases0_library, method):
    tex = T.textures()
    cfg = B.ladder_for_frame(*LADDERS[1])

    def run():
        out = []
        for u in scenes(method)[:4]:
            rp = B.RayPass(cfg, device=0, counters=True, frames_in_flight=1)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            rp.render(); rp.sync()
            out.append((rp.read_hdr().copy(), rp.counters()))
            rp.close()
        return out
    a, b = both(phases0_library, run)
    same_bytes([x[0] for x in a], [x[0] for x in b], f"counting ctx, method {method}")
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1], f"scene {i}: frame counters differ: {x[1]} vs {y[1]}"


@pytest.mark.parametrize("method", [0, 1])
def test_pow13_on_the_device_keeps_directions_and_classes_and_the_colour_bar(method):
    """bh_pow_1p3 on the device (libbhray_pow13.so, `make pow13`: -DBHRAY_POW13=2, the latency no-mesh builds; what ships keeps powf): against the shipped library on one
    frame slot, classes and direction pixels are the same bytes and NaNs fall on the same words; colour channels agree within the project's bar (1e-4 relative,
    magnitudes under 1e-3 absolutely: tests/common.py) - the two powers are 0.5 and 1-2 ulp from the real one - and some colour word does differ (the form is in use)."""
    from bhusie_amd import _lib, layouts
    L = C.CDLL(T.variant_library("pow13"))
    layouts.declare(L)
    saved = _lib.lib()
    tex = T.textures()
    cases = [(B.ladder_for_frame(*LADDERS[1]), u, dict(frames_in_flight=1, speculative_levels=0)) for u in scenes(method)[:4]]
    try:
        a = frames_of(cases, tex)
        _lib._lib = L
        b = frames_of(cases, tex)
    finally:
        _lib._lib = saved
    differ = 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[..., 3], y[..., 3]), f"case {i}: classes differ"
        d = x[..., 3] == 0.0
        assert np.array_equal(x[d].view(np.uint32), y[d].view(np.uint32)), f"case {i}: direction pixels differ"
        assert np.array_equal(np.isnan(x), np.isnan(y)), f"case {i}: NaNs on different words"
        fin = np.isfinite(x).all(axis=-1)
        e = T.rel_err(y[fin], x[fin])
        print(f"method {method}, case {i}: largest colour difference {float(e.max(initial=0.0)):.3g} relative")
        assert float(e.max(initial=0.0)) <= T.REL_TOL
        differ += int((x[fin].view(np.uint32) != y[fin].view(np.uint32)).sum())
    assert differ > 0, "no colour word differs: bh_pow_1p3 is not what the pow13 library runs"


def test_selftest_with_the_phases_legs(phases0_library):
    """bhray_selftest on the device: the legs of the composed sequences count into [0] (every byte through unorm8_rn, two_over_rn) and [1] (dist_rsqrt_rn, normalize_ph):
    no mismatch against the IEEE forms in the shipped library; phases0's kernel runs the same legs."""
    def run():
        rp = B.RayPass(B.ladder_from_base((24, 14), 3, 2), device=0)
        r = rp.selftest()
        rp.close()
        return r
    a, b = both(phases0_library, run)
    assert a == (0, 0, 0), a
    assert b == (0, 0, 0), b
