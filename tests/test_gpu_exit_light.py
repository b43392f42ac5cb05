"""-m gpu: the dense Cash-Karp step behind its third-order bound (bhray_kernels.hip, next_ray_rk_t's SKIP 3 / BHRAY_ERR_SKIP bit 3: when every active lane of a wave has
(dist + 1) |s*h| <= 0.129 the step takes h * 1.0001 without forming e = sum DB_i K_i; the proof stands above the function, its own test is tests/test_err_bound3_cpu.py)
against the kernels before it - the same sources built with -DBHRAY_ERR_SKIP=1 (`make -C bhusie_amd/csrc exit0` -> libbhray_exit0.so, built by __graft_entry__.build();
test infrastructure: R11.1's bound, the parent's kernel text function by function).  The step size a skipped estimate leaves is the one the full text computes, so every
frame must be the same BYTES whichever library marched - but for the sign of a NaN that both frames hold (bench.py's differing_pixels).  The scenes are
the ones in which the march leaves through its rare path in every way it can: iteration limits on both steps of a pair, a camera outside the sphere, feather 0 (a division
by zero in the exit's mix), a step that leaves the sphere and crosses the disk at once, batches, row partitions, temporal speculation, a moving time - on the dense builds
(BHRAY_TRACE_DENSE=1: the ones that changed) and the latency builds, on one frame slot and on 22.  The round's other part - an arm of its own for waves that only leave the
sphere - lost on the clock and did not ship (profiles/EXPERIMENTS.md R19.1); the file keeps the name the round gave it."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T
from tests import test_gpu_step_forms as SF

pytestmark = pytest.mark.gpu

OFF = (1.5, -0.75, 2.0)
OUTSIDE = dict(position=(0.0, 3.0, -45.0), forward=(0.0, -3.0 / 45.1, 45.0 / 45.1), fov=1.0)      # a camera outside the sphere: flat -> relativity -> flat
WORK_SPREAD = 723.0 / 1548406.0        # profiles/EXPERIMENTS.md R9.1: the larger of the two spreads of wave-steps per frame it recorded over three repeats (0.047 %)


def _load(target):
    from bhusie_amd import layouts
    L = C.CDLL(T.variant_library(target))
    layouts.declare(L)
    return L


@pytest.fixture
def exit0_library():
    from bhusie_amd import _lib
    saved = _lib.lib()
    L = _load("exit0")

    def use(exit0: bool):
        _lib._lib = L if exit0 else saved
    yield use
    _lib._lib = saved


def both(exit0_library, fn):
    exit0_library(False); a = fn()
    exit0_library(True); b = fn()
    exit0_library(False)
    return a, b


def same_bytes(a, b, what):
    """bit for bit, except the sign of a NaN both frames hold (bench.py's differing_pixels)"""
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape
        nx, ny = np.isnan(x), np.isnan(y)
        wx, wy = x.view(np.uint32).copy(), y.view(np.uint32).copy()
        wx[nx & ny] = 0; wy[nx & ny] = 0
        d = wx != wy
        assert not d.any(), f"{what}, case {i}: {int(d.any(axis=-1).sum())} pixels differ between the shipped library and the stand-in, first at {np.argwhere(d.any(axis=-1))[:3].tolist()}"


def rk(**kw):
    return T.uniforms(integration_method=1, **kw)


def run(cases, tex, builds=None):
    """cases: (cfg, [uniforms of the frames, in order], RayPass keywords) -> every frame of every case"""
    frames = []
    for cfg, seq, kw in cases:
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        for u in seq:
            rp.set_uniforms(*u)
            rp.render()
            if kw.get("frames_per_batch", 0) <= 1:
                rp.sync()
                frames.append(rp.read_hdr().copy())
        rp.sync()
        if kw.get("frames_per_batch", 0) > 1:
            frames.append(rp.read_hdr().copy())
        if builds is not None:
            builds.append(rp.trace_builds())
        rp.close()
    return frames


def scene_cases(slots):
    cfg = B.ladder_from_base((24, 14), 3, 3)
    s = dict(frames_in_flight=slots)
    cases = [(cfg, [rk()], dict(speculative_levels=0, **s)),                                             # case 0: the hole at +0 - the ORIGIN builds
             (cfg, [rk(black_hole=B.BlackHole(position=OFF))], dict(speculative_levels=0, **s)),          # case 1: off the origin - the general builds
             (cfg, [rk()], dict(speculative_levels=2, **s)),
             (cfg, [rk(black_hole=B.BlackHole(position=OFF))], dict(speculative_levels=2, **s))]
    cases += [(cfg, [rk(max_iterations=mi)], dict(**s)) for mi in (0, 1, 2, 5, 6, 7, 40, 41)]              # the limit and the exit on the same step, on both pair parities
    cases.append((cfg, [rk(camera=B.Camera(**OUTSIDE))], dict(**s)))
    cases.append((cfg, [rk(camera=B.Camera(**OUTSIDE), black_hole=B.BlackHole(position=OFF))], dict(speculative_levels=2, **s)))
    cases.append((cfg, [rk(black_hole=B.BlackHole(feather_amount=0.0))], dict(**s)))                       # 0 / 0 in the exit's mix: the same inf / NaN must come out
    cases.append((cfg, [rk(step_size=2.0)], dict(**s)))                                                   # the exiting segment also crosses the disk
    cases.append((cfg, [rk(step_size=2.0, black_hole=B.BlackHole(position=OFF))], dict(speculative_levels=2, **s)))
    cases.append((cfg, [rk(step_size=1.0), rk(step_size=1.0, black_hole=B.BlackHole(position=OFF))], dict(frames_per_batch=2, frames_in_flight=max(2, slots))))      # a batch of two
    cases.append((cfg, [rk(), rk(time=0.5, step_size=2.0)], dict(speculative_levels=2, frames_per_batch=2, frames_in_flight=max(2, slots))))
    moving = [rk(time=k / 60.0) for k in range(3)]
    cases.append((cfg, moving[:2], dict(row_rank=0, row_world=2, stripe_rows=5, **s)))                    # a 2-way row partition's ranks
    cases.append((cfg, moving[:2], dict(row_rank=1, row_world=2, stripe_rows=5, speculative_levels=2, **s)))
    cases.append((cfg, [moving[0]] * 2 + moving, dict(temporal=True, **s)))                               # BHRAY_F_TEMPORAL
    cases.append((cfg, moving, dict(speculative_levels=2, **s)))                                          # a moving time
    cases.append((cfg, [T.uniforms(integration_method=0), T.uniforms(integration_method=0, black_hole=B.BlackHole(position=OFF))], dict(**s)))   # Euler: kernels unchanged
    return cases


@pytest.mark.parametrize("slots", [1, 22])
@pytest.mark.parametrize("dense", [0, 1])
def test_same_bytes_as_the_stand_in(exit0_library, monkeypatch, dense, slots):
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    cases = scene_cases(slots)
    builds = []
    exit0_library(False); a = run(cases, tex, builds)
    exit0_library(True); b = run(cases, tex)
    exit0_library(False)
    same_bytes(a, b, f"dense {dense}, slots {slots}")
    assert builds[0][0] > 0 and builds[0][1] == 0, f"the hole at +0 marches with the ORIGIN builds: {builds[0]}"
    assert builds[1][0] == 0 and builds[1][1] > 0, f"the hole off the origin marches with the general builds: {builds[1]}"


@pytest.mark.parametrize("dense", [0, 1])
def test_fuzz_scenes_against_the_stand_in(exit0_library, monkeypatch, dense):
    """the edge scenes and the 24 seeded scenes of tests/test_gpu_step_forms.py's generator (both integrators)"""
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    scenes = SF.edge_scenes(2) + SF.fuzz_scenes(24, 2)
    a, b = both(exit0_library, lambda: SF.frames_of(scenes, tex, speculative_levels=0))
    same_bytes(a, b, f"fuzz, dense {dense}")


def test_counting_ctx_frame_counters_are_equal(exit0_library):
    """the counting kernels keep their text: the same frames and the same frame counters from both libraries"""
    tex = T.textures()
    cfg = B.ladder_from_base((24, 14), 3, 3)

    def count():
        out = []
        for u in (rk(), rk(step_size=2.0, black_hole=B.BlackHole(position=OFF)), rk(camera=B.Camera(**OUTSIDE))):
            rp = B.RayPass(cfg, device=0, counters=True, frames_in_flight=1)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            rp.render(); rp.sync()
            out.append((rp.read_hdr().copy(), rp.counters(), rp.err_skip()))
            rp.close()
        return out
    a, b = both(exit0_library, count)
    same_bytes([x[0] for x in a], [x[0] for x in b], "counting ctx")
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1], f"scene {i}: frame counters differ: {x[1]} vs {y[1]}"
        # (the counting kernels count R11.1's bound in both libraries; how many wave-steps a frame takes depends on which wave the hardware hands a ray to)
        assert x[2][0] > 0 and y[2][0] > 0 and x[2][2] == 0 and y[2][2] == 0, f"scene {i}: {x[2]} vs {y[2]}"


def test_the_wave_steps_stay_within_the_recorded_spread(exit0_library):
    """Neither bound changes what a wave marches: work() - wave-steps per frame of the 1080p RK frame on 22 slots after 44 frames - of the two libraries, 24 repeats each,
    alternating (which launch a wave's refill lands in depends on the hardware's timing: single runs of ONE library range over 0.11 %, so the means of 24 are compared -
    their difference scatters with a sigma of about 0.012 %), means within the spread R9.1 recorded for that figure."""
    tex = T.textures()
    cfg = B.ladder_for_frame((1920, 1080), 3, 4)
    u = rk()

    def once():
        rp = B.RayPass(cfg, device=0, frames_in_flight=22, speculative_levels=2)
        rp.set_textures(*tex); rp.set_uniforms(*u)
        for _ in range(44):
            rp.render()
        rp.sync()
        ws, _px, n = rp.work()
        rp.close()
        assert n > 0 and ws > 0
        return ws
    new, old = [], []
    for _ in range(24):                       # alternating
        exit0_library(False); new.append(once())
        exit0_library(True); old.append(once())
    exit0_library(False)
    rel = abs(np.mean(new) - np.mean(old)) / np.mean(old)
    print(f"wave-steps per frame: shipped {new}, stand-in {old}; means differ by {rel:.6f} (bar {WORK_SPREAD:.6f})")
    assert rel <= WORK_SPREAD, (new, old)


def test_the_device_counts_no_violation_of_the_third_order_bound(monkeypatch):
    """The measurement build (`make shares`, -DBHRAY_SHARE_LOG) forms the estimate on every step of the dense RK kernels and counts; one 160x90 frame per scene.  No
    lane-step may pass the third-order bound with e_max above the threshold; whole waves pass it, more often than R11.1's; at step size 2 not every wave-step does."""
    from bhusie_amd import _lib
    monkeypatch.setenv("BHRAY_TRACE_DENSE", "1")
    tex = T.textures()
    cfg = B.ladder_for_frame((160, 90), 3, 3)
    saved = _lib.lib()
    L = _load("shares")
    L.bhray_debug_share_log.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    L.bhray_debug_share_log.restype = C.c_int
    out = (C.c_uint64 * 8)()
    got = []
    try:
        _lib._lib = L
        for u in (rk(), rk(step_size=2.0), rk(step_size=2.0, black_hole=B.BlackHole(position=OFF)), rk(camera=B.Camera(**OUTSIDE), step_size=1.0)):
            assert L.bhray_debug_share_log(out, 1) == 0
            rp = B.RayPass(cfg, device=0, frames_in_flight=1)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            rp.render(); rp.sync()
            frame = rp.read_hdr().copy()
            rp.close()
            assert L.bhray_debug_share_log(out, 1) == 0
            got.append((frame, [int(v) for v in out]))
    finally:
        _lib._lib = saved
    for i, (_f, c) in enumerate(got):
        steps, calm2, visits, light, calm3, violations, _fail2, lanes = c
        print(f"scene {i}: wave-steps {steps}, all lanes pass R11.1's bound {calm2}, the third-order bound {calm3}, violations {violations}; rare-region visits {visits}, leaving only {light}; lane-steps {lanes}")
        assert violations == 0, f"scene {i}: {violations} lane-steps pass the third-order bound with e_max above the threshold"
        assert 0 < steps and calm2 <= steps and calm3 <= steps and 0 < visits and light <= visits and 0 < lanes <= 64 * steps
    assert got[0][1][4] > got[0][1][1] > 0, "step size 0.15: the third-order bound holds for no more wave-steps than R11.1's"
    assert got[1][1][4] < got[1][1][0] and got[2][1][4] < got[2][1][0], "step size 2: every wave-step satisfies the bound - the power arm is never reached"
    # the measurement build's frames are the product's
    rp_frames = []
    for u in (rk(), rk(step_size=2.0)):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex); rp.set_uniforms(*u)
        rp.render(); rp.sync()
        rp_frames.append(rp.read_hdr().copy())
        rp.close()
    same_bytes(rp_frames, [got[0][0], got[1][0]], "measurement build")
