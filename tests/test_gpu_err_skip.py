"""-m gpu: the Cash-Karp step that skips its error estimate where a bound proves it idle (bhray_kernels.hip, next_ray_rk_t's SKIP / BHRAY_ERR_SKIP: when every active
lane of a wave has (dist + 1) * (s*h)^2 <= 3.6e-5 the step takes h * 1.0001 without forming e = sum DB_i K_i; the proof stands above the function, the bound's
own test is tests/test_err_bound_cpu.py) against the kernels before it - the same sources built with -DBHRAY_ERR_SKIP=0 (`make -C bhusie_amd/csrc errskip0` ->
libbhray_errskip0.so, built by __graft_entry__.build(); test infrastructure: the estimate on every step).  The step size a skipped estimate leaves is the one the full
text computes, so every frame must be the same BYTES whichever library marched - also where the power arm IS taken (step sizes 1 and 2), i.e. where waves mix lanes
that pass the bound with lanes that do not.  The dense builds - the ones that skip - are forced with BHRAY_TRACE_DENSE=1 (read at create), not by a 1080p frame; the
latency builds are compared too.  A counting ctx reports how often the bound held and, measured on the device, that it never held with an estimate above the threshold."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T

pytestmark = pytest.mark.gpu

OFF = (1.5, -0.75, 2.0)
OUTSIDE = dict(position=(0.0, 3.0, -45.0), forward=(0.0, -3.0 / 45.1, 45.0 / 45.1), fov=1.0)      # a camera outside the sphere: flat -> relativity -> flat
SHAPES = {3: ((192, 108), 3, 3), 4: ((320, 180), 3, 4)}                                           # frame, multiplier, ladder levels


@pytest.fixture
def errskip0_library():
    from bhusie_amd import _lib, layouts
    path = T.variant_library("errskip0")
    saved = _lib.lib()
    L = C.CDLL(path)
    layouts.declare(L)

    def use(errskip0: bool):
        _lib._lib = L if errskip0 else saved
    yield use
    _lib._lib = saved


def both(errskip0_library, fn):
    errskip0_library(False); a = fn()
    errskip0_library(True); b = fn()
    errskip0_library(False)
    return a, b


def same_bytes(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape
        d = x.view(np.uint32) != y.view(np.uint32)
        assert not d.any(), f"{what}, case {i}: {int(d.any(axis=-1).sum())} pixels differ between the shipped library and the stand-in, first at {np.argwhere(d.any(axis=-1))[:3].tolist()}"


def ladder(levels):
    return B.ladder_for_frame(*SHAPES[levels])


def run(cases, tex):
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
        rp.close()
    return frames


def rk(**kw):
    return T.uniforms(integration_method=1, **kw)


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("levels,kw", [(3, dict(speculative_levels=0)), (4, dict(speculative_levels=2, frames_in_flight=1))])
@pytest.mark.parametrize("step_size", [0.15, 1.0, 2.0])
def test_same_bytes_as_the_estimate_on_every_step(errskip0_library, monkeypatch, dense, levels, kw, step_size):
    """Latency and dense builds, 192x108 with 3 ladder levels and 320x180 with 4, speculative levels 0 and 2, the hole at the origin (the ORIGIN builds) and off it (the
    general builds), step sizes 0.15 (the bound holds nearly everywhere), 1 and 2 (the power arm is taken: waves of mixed lanes)."""
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    cfg = ladder(levels)
    cases = [(cfg, [rk(step_size=step_size)], kw), (cfg, [rk(step_size=step_size, black_hole=B.BlackHole(position=OFF))], kw)]
    a, b = both(errskip0_library, lambda: run(cases, tex))
    same_bytes(a, b, f"step_size {step_size}, dense {dense}, {levels} levels, {kw}")


@pytest.mark.parametrize("dense", [0, 1])
def test_iteration_limits_camera_outside_batches_and_temporal(errskip0_library, monkeypatch, dense):
    """Iteration limits 1 / 2 / 7 / 40 (the limit on either step of a pair), a camera outside the sphere (also at step size 2), a batch of two frames (one with the
    hole off the origin, then two at it), BHRAY_F_TEMPORAL over a moving sequence."""
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    cfg = ladder(3)
    cases = [(cfg, [rk(max_iterations=mi)], dict()) for mi in (1, 2, 7, 40)]
    cases.append((cfg, [rk(camera=B.Camera(**OUTSIDE))], dict()))
    cases.append((cfg, [rk(camera=B.Camera(**OUTSIDE), step_size=2.0)], dict(speculative_levels=2, frames_in_flight=1)))
    two = dict(frames_per_batch=2, frames_in_flight=2)
    cases.append((cfg, [rk(step_size=1.0), rk(step_size=1.0, black_hole=B.BlackHole(position=OFF))], two))
    cases.append((cfg, [rk(), rk(time=0.5, step_size=2.0)], dict(speculative_levels=2, **two)))
    moving = [rk(time=k / 60.0, step_size=1.0) for k in range(3)]
    cases.append((cfg, [moving[0]] * 2 + moving, dict(frames_in_flight=1, temporal=True)))
    a, b = both(errskip0_library, lambda: run(cases, tex))
    same_bytes(a, b, f"limits / outside / batches / temporal, dense {dense}")


def test_the_device_counts_no_violation_of_the_bound(errskip0_library):
    """A counting ctx forms the estimate on every step and counts: RK wave-steps, wave-steps whose active lanes all satisfied the bound, lane-steps that satisfied it
    with an estimate above the threshold.  The last must be 0 at every step size; at 0.15 whole waves qualify; at 2.0 not every wave-step does.  The frame and its
    frame counters are the stand-in's, whose library counts nothing."""
    tex = T.textures()
    cfg = ladder(3)

    def count():
        out = []
        for u in (rk(step_size=0.15), rk(step_size=1.0), rk(step_size=2.0), rk(step_size=2.0, black_hole=B.BlackHole(position=OFF)), T.uniforms(integration_method=0)):
            rp = B.RayPass(cfg, device=0, counters=True, frames_in_flight=1)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            rp.render(); rp.sync()
            out.append((rp.read_hdr().copy(), rp.counters(), rp.err_skip()))
            rp.close()
        return out
    a, b = both(errskip0_library, count)
    same_bytes([x[0] for x in a], [x[0] for x in b], "counting ctx")
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1], f"scene {i}: frame counters differ: {x[1]} vs {y[1]}"
        assert y[2] == (0, 0, 0), f"scene {i}: the stand-in counts nothing: {y[2]}"
        print(f"scene {i}: (wave-steps, all lanes pass, violations) = {x[2]}")
    for i in range(4):
        steps, calm, violations = a[i][2]
        assert violations == 0, f"scene {i}: {violations} lane-steps satisfied the bound with e_max above the threshold"
        assert 0 < steps and calm <= steps
    assert a[0][2][1] > 0, "step size 0.15: no wave-step on which every active lane satisfied the bound"
    assert a[2][2][1] < a[2][2][0] and a[3][2][1] < a[3][2][0], "step size 2: every wave-step satisfied the bound - the power arm is never reached"
    assert a[4][2] == (0, 0, 0), "Euler has no error estimate"
