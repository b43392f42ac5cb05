"""-m gpu: the ORIGIN builds of the no-mesh contract trace kernels (bhray_kernels.hip, trace_kernel's ORIGIN: the hole's position the constant +0 vector, the unified
pairs without position - bpos; chosen by the host per launch when every frame of the batch has the hole at +0, +0, +0) against the kernels before them - the same
sources built with -DBHRAY_ORIGIN_KERNEL=0 (`make -C bhusie_amd/csrc origin0` -> libbhray_origin0.so, built by __graft_entry__.build(); test infrastructure: the
wave-uniform test inside the Euler kernels, nothing in the RK kernels).  x - (+0) is x for every x, so every frame must be the same BYTES whichever build marched;
WHICH build marched is read from bhray_get_trace_builds, not from a clock.  The dense builds are forced with BHRAY_TRACE_DENSE=1 (read at create), not by a 1080p frame."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T

pytestmark = pytest.mark.gpu

OFF = (1.5, -0.75, 2.0)
MINUS_ZERO = (-0.0, 0.0, 0.0)
OUTSIDE = dict(position=(0.0, 3.0, -45.0), forward=(0.0, -3.0 / 45.1, 45.0 / 45.1), fov=1.0)      # a camera outside the sphere: flat -> relativity -> flat


@pytest.fixture
def origin0_library():
    from bhusie_amd import _lib, layouts
    path = T.variant_library("origin0")
    saved = _lib.lib()
    L = C.CDLL(path)
    layouts.declare(L)

    def use(origin0: bool):
        _lib._lib = L if origin0 else saved
    yield use
    _lib._lib = saved


def both(origin0_library, fn):
    origin0_library(False); a = fn()
    origin0_library(True); b = fn()
    origin0_library(False)
    return a, b


def same_bytes(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape
        d = x.view(np.uint32) != y.view(np.uint32)
        assert not d.any(), f"{what}, case {i}: {int(d.any(axis=-1).sum())} pixels differ between the ORIGIN builds' library and the stand-in, first at {np.argwhere(d.any(axis=-1))[:3].tolist()}"


def run(cases, tex, every_frame=False):
    """cases: (cfg, [uniforms of the frames, in order], RayPass keywords) -> per case (frames read, (ORIGIN launches, other launches)); the last frame, or every frame"""
    frames, builds = [], []
    for cfg, seq, kw in cases:
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        per_frame = []
        for u in seq:
            rp.set_uniforms(*u)
            rp.render()
            if every_frame:
                rp.sync()
                frames.append(rp.read_hdr().copy())
                per_frame.append(rp.trace_builds())
        rp.sync()
        if not every_frame:
            frames.append(rp.read_hdr().copy())
        builds.append(per_frame if every_frame else rp.trace_builds())
        rp.close()
    return frames, builds


def ladder(levels):
    return B.ladder_from_base((20, 12) if levels == 2 else (10, 6), 3, levels)      # the shapes of tests/test_gpu_step_forms.py


def hole(position, **kw):
    return B.BlackHole(position=position, **kw)


def origin_scenes(method, levels):
    """the hole at +0: the exits where the hole-relative position is written on leaving the march - the iteration limit on either step of a pair and before the first,
    the sphere's surface from inside and from a camera outside it, feather 0 (NaN directions) - and a disk outside the sphere"""
    cfg = ladder(levels)
    sc = [(cfg, [T.uniforms(integration_method=method)])]
    for mi in (0, 1, 2, 5, 6, 7, 40, 41):
        sc.append((cfg, [T.uniforms(integration_method=method, max_iterations=mi)]))
    sc.append((cfg, [T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE))]))
    sc.append((cfg, [T.uniforms(integration_method=method, black_hole=B.BlackHole(feather_amount=0.0))]))
    sc.append((cfg, [T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE), black_hole=B.BlackHole(relativity_sphere_radius=9.0, accretion_disk_outer=14.0))]))
    return sc


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("levels,kw", [(2, dict(speculative_levels=0)), (3, dict(speculative_levels=2, frames_in_flight=1))])
def test_hole_at_the_origin_takes_the_origin_build_with_the_same_bytes(origin0_library, monkeypatch, method, dense, levels, kw):
    """RK and Euler, latency and dense build, speculative levels 0 and 2, the hole at +0: every trace launch of the shipped library gets an ORIGIN build, none of the
    stand-in's does, and the frames are the same bytes."""
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    cases = [(cfg, seq, kw) for cfg, seq in origin_scenes(method, levels)]
    (a, ba), (b, bb) = both(origin0_library, lambda: run(cases, tex))
    same_bytes(a, b, f"hole at +0, method {method}, dense {dense}, {kw}")
    for i, (x, y) in enumerate(zip(ba, bb)):
        assert x[0] > 0 and x[1] == 0, f"case {i}: (ORIGIN, other) launches {x}: every trace launch of a frame with the hole at +0 takes the ORIGIN build"
        assert y[0] == 0 and y[1] == x[0], f"case {i}: the stand-in has no ORIGIN build: {y} against {x}"


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("dense", [0, 1])
def test_minus_zero_and_off_origin_take_the_general_build(origin0_library, monkeypatch, method, dense):
    """A single -0 component is not the origin (x - (-0) is not x for x = -0), nor is a hole elsewhere: the general build, asserted through the ctx's launch counts."""
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    cases = []
    for levels, kw in ((2, dict(speculative_levels=0)), (3, dict(speculative_levels=2, frames_in_flight=1))):
        for pos in (MINUS_ZERO, (0.0, -0.0, 0.0), (0.0, 0.0, -0.0), OFF):
            cases.append((ladder(levels), [T.uniforms(integration_method=method, black_hole=hole(pos))], kw))
            cases.append((ladder(levels), [T.uniforms(integration_method=method, black_hole=hole(pos), camera=B.Camera(**OUTSIDE))], kw))
    (a, ba), (b, bb) = both(origin0_library, lambda: run(cases, tex))
    same_bytes(a, b, f"hole at -0 / off the origin, method {method}, dense {dense}")
    for i, (x, y) in enumerate(zip(ba, bb)):
        assert x[0] == 0 and x[1] > 0, f"case {i}: (ORIGIN, other) launches {x}: the general build must be taken"
        assert y == x


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("dense", [0, 1])
def test_a_batch_with_the_hole_at_and_off_the_origin(origin0_library, monkeypatch, method, dense):
    """frames_per_batch = 2: one launch covers two frames; when only one of them has the hole at the origin the launch is the general build.  Read both ways round (the
    frame read is the batch's last), and two frames at the origin for the ORIGIN build with nb = 2."""
    monkeypatch.setenv("BHRAY_TRACE_DENSE", str(dense))
    tex = T.textures()
    at, off = T.uniforms(integration_method=method), T.uniforms(integration_method=method, black_hole=hole(OFF))
    at2 = T.uniforms(integration_method=method, time=0.5)
    kw = dict(frames_per_batch=2, frames_in_flight=2, speculative_levels=2)
    cases = [(ladder(3), seq, kw) for seq in ([at, off], [off, at], [at, at2])] + [(ladder(2), seq, dict(frames_per_batch=2, frames_in_flight=2)) for seq in ([at, off], [off, at], [at, at2])]
    (a, ba), (b, bb) = both(origin0_library, lambda: run(cases, tex))
    same_bytes(a, b, f"batches of two, method {method}, dense {dense}")
    for i, x in enumerate(ba):
        if i % 3 == 2: assert x[0] > 0 and x[1] == 0, f"case {i}: both frames at the origin: {x}"
        else: assert x[0] == 0 and x[1] > 0, f"case {i}: one frame of the batch off the origin: {x}"


@pytest.mark.parametrize("method", [0, 1])
def test_the_hole_moves_off_the_origin_and_back(origin0_library, method):
    """A ctx with several frame slots, the hole off the origin and back between frames: the build changes per launch, every frame is the stand-in's."""
    tex = T.textures()
    pos = [(0.0, 0.0, 0.0), OFF, (0.0, 0.0, 0.0), MINUS_ZERO, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.25, 0.0, 0.0)]
    seq = [T.uniforms(integration_method=method, black_hole=hole(p), time=k / 60.0) for k, p in enumerate(pos)]
    cases = [(ladder(3), seq, dict(frames_in_flight=3, speculative_levels=2)), (ladder(2), seq, dict(frames_in_flight=4))]
    (a, ba), (b, bb) = both(origin0_library, lambda: run(cases, tex, every_frame=True))
    same_bytes(a, b, f"moving hole, method {method}")
    for per_frame in ba:
        prev = (0, 0)
        for p, now in zip(pos, per_frame):
            d = (now[0] - prev[0], now[1] - prev[1])
            at_origin = all(np.float32(v).view(np.uint32) == 0 for v in p)
            assert (d[0] > 0 and d[1] == 0) if at_origin else (d[0] == 0 and d[1] > 0), f"hole at {p}: (ORIGIN, other) launches of this frame {d}"
            prev = now
    for per_frame in bb:
        assert all(n[0] == 0 for n in per_frame)


@pytest.mark.parametrize("method", [0, 1])
def test_temporal_partition_and_quad_march(origin0_library, method):
    """BHRAY_F_TEMPORAL (the predicted launch is a dense build, the fix-up launches latency builds), one rank of a 2-way row partition, and a one-slot ctx small enough
    for the quad march (bhray_quad.inc: its hole position comes from the same constants), all with the hole at +0 - and the quad march with the hole off it."""
    tex = T.textures()
    moving = [T.uniforms(integration_method=method, time=k / 60.0) for k in range(4)]
    cases = [(ladder(3), [moving[0]] * 3 + moving, dict(frames_in_flight=1, temporal=True)),
             (ladder(2), [moving[0]] * 2 + moving, dict(frames_in_flight=2, temporal=True)),
             (ladder(2), moving[:2], dict(frames_in_flight=1, row_rank=1, row_world=2, stripe_rows=5)),
             (ladder(3), moving[:2], dict(frames_in_flight=2, row_rank=0, row_world=2, stripe_rows=9, speculative_levels=2)),
             (B.ladder_from_base((10, 6), 3, 3), moving[:1], dict(frames_in_flight=1)),                        # short queues on one slot: quads
             (B.ladder_from_base((10, 6), 3, 2), [T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE))], dict(frames_in_flight=1))]
    (a, ba), (b, bb) = both(origin0_library, lambda: run(cases, tex))
    same_bytes(a, b, f"temporal / partition / quads, method {method}")
    for i, (x, y) in enumerate(zip(ba, bb)):
        assert x[0] > 0 and x[1] == 0, f"case {i}: {x}"
        assert y[0] == 0 and y[1] == x[0], f"case {i}: {y} against {x}"
    off = [(B.ladder_from_base((10, 6), 3, 3), [T.uniforms(integration_method=method, black_hole=hole(OFF))], dict(frames_in_flight=1))]
    (a, ba), (b, bb) = both(origin0_library, lambda: run(off, tex))
    same_bytes(a, b, f"quads, hole off the origin, method {method}")
    assert ba[0][0] == 0 and ba[0][1] > 0


@pytest.mark.parametrize("method", [0, 1])
def test_the_environment_override_never_takes_the_origin_build(monkeypatch, method):
    """BHRAY_ORIGIN_KERNEL=0 at create (the A/B's switch): the general build for a hole at +0, the same bytes as with it."""
    tex = T.textures()
    cases = [(ladder(3), [T.uniforms(integration_method=method)], dict(speculative_levels=2, frames_in_flight=1)), (ladder(2), [T.uniforms(integration_method=method)], dict())]
    a, ba = run(cases, tex)
    monkeypatch.setenv("BHRAY_ORIGIN_KERNEL", "0")
    b, bb = run(cases, tex)
    same_bytes(a, b, f"BHRAY_ORIGIN_KERNEL=0, method {method}")
    for x, y in zip(ba, bb):
        assert x[0] > 0 and x[1] == 0 and y[0] == 0 and y[1] == x[0], (x, y)


@pytest.mark.parametrize("method", [0, 1])
def test_a_counting_ctx_never_takes_the_origin_build(origin0_library, method):
    """The kernels that count have no ORIGIN build: the same frame counters and the same bytes as before."""
    tex = T.textures()
    cfg = ladder(2)

    def count():
        out = []
        for u in (T.uniforms(integration_method=method), T.uniforms(integration_method=method, camera=B.Camera(**OUTSIDE))):
            rp = B.RayPass(cfg, device=0, counters=True, frames_in_flight=1)
            rp.set_textures(*tex); rp.set_uniforms(*u)
            rp.render(); rp.sync()
            out.append((rp.read_hdr().copy(), rp.counters(), rp.trace_builds()))
            rp.close()
        return out
    a, b = both(origin0_library, count)
    same_bytes([x[0] for x in a], [x[0] for x in b], f"counting ctx, method {method}")
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1], f"scene {i}: frame counters differ: {x[1]} vs {y[1]}"
        assert x[2][0] == 0 and x[2][1] > 0 and y[2] == x[2], (x[2], y[2])
