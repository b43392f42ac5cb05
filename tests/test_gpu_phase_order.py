"""-m gpu: the ORDER of a round's phases in the trace kernels (BHRAY_PHASE_ORDER, bhray_kernels.hip: refill, march, shade, flat - with the general step and a second
flat pass behind it in the no-mesh contract RK kernels -, epilogue) against the earlier order (refill, shade, flat, epilogue, march) - the same sources built with
-DBHRAY_PHASE_ORDER=0 (`make -C bhusie_amd/csrc phase0` -> libbhray_phase0.so, built by __graft_entry__.build(); test infrastructure, and the earlier kernels'
instructions exactly).  The order is scheduling only - every ray executes the same operations on the same values in the same order - so every frame must be the
same BYTES (but the sign of a NaN) and every frame counter equal; what changes is how many wave-steps the trace waves issue for them, and the last test
holds the new order to issuing fewer."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T

pytestmark = pytest.mark.gpu


@pytest.fixture
def phase0_library():
    from bhusie_amd import _lib, layouts
    path = T.variant_library("phase0")
    saved = _lib.lib()
    L = C.CDLL(path)
    layouts.declare(L)

    def use(phase0: bool):
        _lib._lib = L if phase0 else saved
    yield use
    _lib._lib = saved


def same_bytes(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape
        both_nan = np.isnan(x) & np.isnan(y)
        xa, ya = np.where(both_nan, 0.0, x).astype(np.float32), np.where(both_nan, 0.0, y).astype(np.float32)
        d = xa.view(np.uint32) != ya.view(np.uint32)
        assert not d.any(), f"{what}, case {i}: {int(d.any(axis=-1).sum())} pixels differ between the two phase orders, first at {np.argwhere(d.any(axis=-1))[:3].tolist()}"


def frames_of(cases, tex, model=None):
    """cases: (cfg, [uniforms of the frames, in order], RayPass keywords); the last frame of each"""
    out = []
    for cfg, seq, kw in cases:
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        if model is not None:
            rp.upload_model(model)
        for u in seq:
            rp.set_uniforms(*u)
            rp.render()
        rp.sync()
        out.append(rp.read_hdr().copy())
        rp.close()
    return out


def both(phase0_library, fn):
    phase0_library(False); a = fn()
    phase0_library(True); b = fn()
    phase0_library(False)
    return a, b


OUTSIDE = dict(position=(0.0, 3.0, -45.0), forward=(0.0, -3.0 / 45.1, 45.0 / 45.1), fov=1.0)      # a camera outside the sphere: flat -> relativity -> flat


def small_scenes(method, **extra):
    return [T.uniforms(integration_method=method, **extra),
            T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE), **extra),
            T.uniforms(integration_method=method, max_iterations=41, **extra),                                     # the iteration limit inside the march, odd and even
            T.uniforms(integration_method=method, max_iterations=291, step_size=0.05, **extra),
            T.uniforms(integration_method=method, black_hole=B.BlackHole(feather_amount=0.0), **extra),            # NaN directions at the exit
            T.uniforms(integration_method=method, black_hole=B.BlackHole(position=(3.0, -2.0, 5.0)), **extra),     # hole off the origin
            T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE), black_hole=B.BlackHole(relativity_sphere_radius=9.0, accretion_disk_outer=14.0), **extra)]   # disk outside the sphere


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("spec", [0, 2])
def test_one_frame_slot_latency_builds_thin_and_quad_launches(phase0_library, method, spec):
    """One frame slot: the latency builds; the coarse levels' short queues are dealt out as thin shares and marched by quads (bhray_quad.inc), the last level pulls
    from the queue head."""
    tex = T.textures()
    cases = []
    for cfg in (B.ladder_from_base((10, 6), 3, 3), B.ladder_from_base((24, 14), 3, 4), B.ladder_for_frame((320, 180), 3, 3)):
        cases += [(cfg, [u], dict(frames_in_flight=1, speculative_levels=spec)) for u in small_scenes(method)]
    a, b = both(phase0_library, lambda: frames_of(cases, tex))
    same_bytes(a, b, f"one slot, method {method}, speculative levels {spec}")


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("spec", [0, 2])
def test_22_frame_slots_dense_builds(phase0_library, method, spec):
    """A full set of frame slots at 1920x1080: the dense builds; the last of 24 frames."""
    tex = T.textures()
    cfg = B.ladder_for_frame((1920, 1080), 3, 4)
    kw = dict(frames_in_flight=22, speculative_levels=spec)
    cases = [(cfg, [T.uniforms(integration_method=method)] * 24, kw),
             (cfg, [T.uniforms(integration_method=method, max_iterations=301, camera=B.Camera(position=(2.0, 1.0, -25.0), forward=(-0.08, -0.04, 1.0), fov=1.3))] * 24, kw),
             (cfg, [T.uniforms(integration_method=method, black_hole=B.BlackHole(position=(1.5, -0.75, 2.0)))] * 24, kw),
             (cfg, [T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE))] * 24, kw)]
    a, b = both(phase0_library, lambda: frames_of(cases, tex))
    same_bytes(a, b, f"22 slots, method {method}, speculative levels {spec}")


@pytest.mark.parametrize("method", [0, 1])
def test_batches_row_partition_temporal_and_moving_time(phase0_library, method):
    tex = T.textures()
    cfg = B.ladder_from_base((24, 14), 3, 4)
    big = B.ladder_for_frame((640, 360), 3, 4)
    moving = [T.uniforms(integration_method=method, time=k / 60.0) for k in range(7)]                   # the disk turns from frame to frame
    cases = [(cfg, moving, dict(frames_in_flight=2, frames_per_batch=3, speculative_levels=2)),         # batches: nb > 1 in every launch
             (big, moving, dict(frames_in_flight=4, frames_per_batch=2)),
             (big, moving, dict(frames_in_flight=22, speculative_levels=2)),
             (big, moving[:3], dict(frames_in_flight=1, row_rank=1, row_world=3, stripe_rows=9)),       # a row partition's rank
             (big, moving[:3], dict(frames_in_flight=3, row_rank=0, row_world=2, stripe_rows=27, speculative_levels=2)),
             (cfg, [moving[0]] * 3 + moving, dict(frames_in_flight=1, temporal=True)),                  # BHRAY_F_TEMPORAL: predicted launches + fix-up launches on nearly empty queues
             (big, [moving[0]] * 3 + moving, dict(frames_in_flight=2, temporal=True))]
    a, b = both(phase0_library, lambda: frames_of(cases, tex))
    same_bytes(a, b, f"batches / partition / temporal / time, method {method}")


@pytest.mark.parametrize("method", [0, 1])
def test_mesh_workload(phase0_library, tmp_path, method):
    """The mesh variant's kernels get the rotation alone (their flat phase keeps its own batching rule): the latency build and the dense, parked build."""
    from bhusie_amd import assets
    tex = T.textures()
    p = tmp_path / "mesh.obj"
    p.write_text(assets.icosphere_mesh_obj(3, radius=6.0, bump=0.2, seed=11))
    model = B.load_model(str(p))
    model.set_transform((-7.0, 1.0, 24.0), 1)
    small = B.ladder_from_base((24, 14), 3, 2)
    big = B.ladder_for_frame((1920, 1080), 3, 4)
    cases = [(small, [T.uniforms(integration_method=method, model_count=1)], dict(speculative_levels=0)),
             (small, [T.uniforms(integration_method=method, model_count=1, camera=B.Camera(**OUTSIDE))], dict(speculative_levels=0)),
             (big, [T.uniforms(integration_method=method, model_count=1)] * 24, dict(frames_in_flight=22, speculative_levels=2))]
    a, b = both(phase0_library, lambda: frames_of(cases, tex, model=model))
    same_bytes(a, b, f"mesh workload, method {method}")


@pytest.mark.parametrize("method", [0, 1])
def test_counting_ctx_frame_counters_are_equal(phase0_library, method):
    """A counting ctx (the kernels that count march with the general step): counters() - the counters that are a property of the frame - equal; the wave-step
    diagnostic (scheduling_counters) is what the order changes."""
    tex = T.textures()
    cfg = B.ladder_for_frame((320, 180), 3, 4)

    def run():
        out = []
        for u in (T.uniforms(integration_method=method), T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE))):
            rp = B.RayPass(cfg, device=0, counters=True, frames_in_flight=1)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            rp.render(); rp.sync()
            out.append((rp.read_hdr().copy(), rp.counters(), rp.scheduling_counters()))
            rp.close()
        return out
    a, b = both(phase0_library, run)
    same_bytes([x[0] for x in a], [x[0] for x in b], f"counting ctx, method {method}")
    for i, (x, y) in enumerate(zip(a, b)):
        print(f"counting ctx, method {method}, scene {i}: scheduling counters {x[2]} | phase0 {y[2]}")
        assert x[1] == y[1], f"scene {i}: frame counters differ: {x[1]} vs {y[1]}"


def test_the_new_order_issues_fewer_wave_steps(phase0_library):
    """The mechanism, without a clock: the wave-steps the trace waves issue (bhray_get_work: counted in every build, in whole batches where the step loop is entered)
    for the 1080p RK frame on 22 slots, after the same number of frames.  The new order must issue fewer than the earlier one, by more than the earlier order's own
    spread over three repeats (which launch a wave's refill lands in depends on the hardware's timing)."""
    tex = T.textures()
    cfg = B.ladder_for_frame((1920, 1080), 3, 4)
    u = T.uniforms(integration_method=1)

    def run():
        out = []
        for _ in range(3):
            rp = B.RayPass(cfg, device=0, frames_in_flight=22, speculative_levels=2)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            for _ in range(44):
                rp.render()
            rp.sync()
            ws, _px, n = rp.work()
            out.append(ws)
            assert n > 0 and ws > 0
            rp.close()
        return out
    new, old = both(phase0_library, run)
    spread = max(old) - min(old)
    print(f"wave-steps per frame: new order {new}, phase0 {old}; ratio of means {np.mean(new) / np.mean(old):.4f}; phase0's spread {spread:.1f} ({spread / np.mean(old):.5f})")
    assert max(new) < min(old) - spread, (new, old)
