"""-m gpu: lensed meshes (bhray_set_mesh_lensing) - models tested on every integrator step inside the relativity sphere.

The reference is tests/lensed_ref.py: oracle.np_ray's trace_rays with the one literal of ray.wgsl:541 changed.  It runs live on the CPU
(seconds per scene, cached per scene); the GPU work is milliseconds.  Frames are tiny (32x18, or ladders from a 16x9 base) and the mesh is
an 80-triangle icosphere.  Comparison: tests/common.assert_parity (classes identical, channels within REL_TOL), direction pixels bit
for bit, and steps / traced / sky_samples of a counting ctx equal to the reference's.  A test hides nothing: every named scene must show
at least 5 segments on which a model won IN THE REFERENCE, the named scenes together at least 50.
"""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from oracle import np_ray as N
from tests import common as T
from tests import lbvh_ref as LB
from tests import lensed_ref as LR

pytestmark = pytest.mark.gpu

ONE = ((32, 18),)
LADDER2 = ((16, 9), (46, 25))
LADDER3 = ((16, 9), (46, 25), (136, 73))
OUTSIDE = (0.0, 3.0, -45.0)
CAM_OUT = (OUTSIDE, tuple(float(v) for v in -np.array(OUTSIDE) / np.linalg.norm(OUTSIDE)), 0.5)   # towards the origin
FINER = ((48, 27),)
# name: (camera | None = the default one, [(mesh radius, mesh position, visible)], frame)
# The last scene at 32x18 shows 12 segment hits with Euler but 3 with RK (RK integrates from the camera outside the sphere while the hit tests start at the entry point, so
# most of its rays meet the mesh in flat space): it is rendered at 48x27 - the same scene, sampled more densely - where the reference shows 8 (RK) and 28 (Euler).
SCENES = {
    "front_beside_the_hole": (None, [(3, (3.5, -1.5, -8.0), 1)], ONE),
    "behind_the_hole": (None, [(7, (0.5, 2.0, 11.0), 1)], ONE),
    "straddling_R": (None, [(8, (-10.0, 0.0, 17.0), 1)], ONE),
    "camera_outside": (CAM_OUT, [(5, (5.0, 1.0, -6.0), 1)], ONE),
    "camera_outside_straddling_R": (CAM_OUT, [(8, (-8.0, 0.0, -17.0), 1)], FINER),
}
MIN_HITS = 5           # per named scene, on the reference's own count
MIN_HITS_TOGETHER = 50


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _mesh_dir():
    d = tempfile.mkdtemp(prefix="lensed_meshes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _model(radius, pos, visible=1, sah=False):
    p = os.path.join(_mesh_dir(), f"ico1_{radius}.obj")
    if not os.path.exists(p):
        with open(p, "w") as f:
            f.write(assets.icosphere_mesh_obj(1, radius=float(radius)))       # 80 triangles
    m = B.load_model(p)
    if sah:
        m.build_bvh_sah()
    m.set_transform(pos, visible)
    return m


def _uniforms(cam, method, count, hole=None, **details):
    camera = B.Camera(position=cam[0], forward=cam[1], fov=cam[2]) if cam else None
    bh = B.BlackHole(position=hole) if hole else None
    return T.uniforms(camera=camera, black_hole=bh, integration_method=method, model_count=count, **details)


@functools.lru_cache(maxsize=None)
def _reference(cam, models, method, sizes, hole=None):
    """(levels, stats) of tests/lensed_ref.py for one scene; computed once, shared, never written to"""
    u = _uniforms(cam, method, len(models), hole)
    S = N.Scene(*u, *T.textures(), [_model(*m).arrays() for m in models])
    st = {}
    imgs = LR.render_ladder_lensed(S, [tuple(s) for s in sizes], st)
    for i in imgs:
        i.setflags(write=False)
    return imgs, st


def _cfg(sizes):
    cfg = B.ladder_from_base(sizes[0], 3, len(sizes))
    assert [tuple(s) for s in cfg.sizes()] == [tuple(s) for s in sizes]
    return cfg


def _ctx(sizes, models, lensed=True, lib=None, build=False, **kw):
    rp = B.RayPass(_cfg(sizes), **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*T.textures())
    for i, m in enumerate(models):
        if m is not None:
            (rp.upload_model_build if build else rp.upload_model)(_model(*m) if isinstance(m, tuple) else m, i)
    if lensed:
        rp.set_mesh_lensing(1)
    return rp


def _check(rp, want, what, levels=True):
    """every level (or the frame) against the reference: parity, direction pixels bit for bit"""
    imgs = [rp.read_level(l) for l in range(len(want))] if levels else [rp.read_hdr()]
    for l, (got, w) in enumerate(zip(imgs, want if levels else want[-1:])):
        T.assert_parity(got, w, f"{what} level {l}")
        d = w[..., 3] == 0
        assert np.array_equal(_bits(got[d]), _bits(w[d])), f"{what} level {l}: direction pixels must be bit-identical"


def _check_counters(rc, stats, what):
    c = rc.counters()
    print(what, "counters", {k: c[k] for k in ("steps", "traced", "sky_samples")}, "reference", stats)
    for k in ("steps", "traced", "sky_samples"):
        assert c[k] == stats[k], (what, k, c[k], stats[k])


# ---- 1. scenes, both integrators
@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_scene_matches_the_reference(scene, method):
    cam, models, size = SCENES[scene]
    models = tuple(models)
    want, st = _reference(cam, models, method, size)
    print(scene, method, st)
    # the floor, on the reference's own count, for every scene with every integrator.  Measured (RK / Euler): 14 / 14, 31 / 37, 11 / 11, 7 / 16, 8 / 28.
    assert st["segment_hits"] >= MIN_HITS, (scene, st)
    u = _uniforms(cam, method, len(models))
    rp = _ctx(size, models)
    rp.set_uniforms(*u); rp.render()
    lensed = rp.read_hdr().copy()
    _check(rp, want, f"{scene} method {method}")
    if scene == "front_beside_the_hole":
        # the same ctx with the mode off: the model inside the sphere is not in that frame (this is what fails without the feature)
        rp.set_mesh_lensing(0); rp.render()
        off = rp.read_hdr()
        assert int((_bits(off) != _bits(lensed)).any(axis=-1).sum()) >= 10
    rp.close()
    rc = _ctx(size, models, counters=True)
    rc.set_uniforms(*u); rc.render()
    _check_counters(rc, st, f"{scene} method {method}")
    _check(rc, want, f"{scene} method {method} counting build", levels=False)
    rc.close()


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_named_scenes_together_hold_enough_segment_hits(method):
    total = sum(_reference(SCENES[s][0], tuple(SCENES[s][1]), method, SCENES[s][2])[1]["segment_hits"] for s in SCENES)
    assert total >= MIN_HITS_TOGETHER, total                  # (71 with RK, 106 with Euler)


# ---- 2. hole off the origin: the general (non-ORIGIN) kernels' path
@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_hole_off_the_origin(method):
    hole = (1.5, -0.5, 2.0)
    # Behind the moved hole.  The default camera is then 21.06 from the hole, outside R = 20: every ray starts in flat space, and with RK (the shader integrates from the
    # camera while its hit tests start at the sphere's entry point) a mesh that a straight line from the camera reaches is found by the flat phase first - a mesh beside
    # the hole shows 0-2 segment hits with RK (14-21 with Euler); behind the hole it is reached by bent rays only.
    models = ((7, (2.0, 1.5, 13.0), 1),)
    want, st = _reference(None, models, method, ONE, hole)
    assert st["segment_hits"] >= MIN_HITS, st
    rp = _ctx(ONE, models, counters=True)
    rp.set_uniforms(*_uniforms(None, method, 1, hole)); rp.render()
    _check(rp, want, f"hole off the origin, method {method}")
    _check_counters(rp, st, "hole off the origin")
    rp.close()


# ---- 3. ladders
BEHIND = ((7, (0.5, 2.0, 11.0), 1),)


def test_two_level_ladder():
    want, st = _reference(None, BEHIND, 1, LADDER2)
    assert st["segment_hits"] >= MIN_HITS, st
    rp = _ctx(LADDER2, BEHIND, counters=True)
    rp.set_uniforms(*_uniforms(None, 1, 1)); rp.render()
    _check(rp, want, "two-level ladder")
    _check_counters(rp, st, "two-level ladder")
    rp.close()


@functools.lru_cache(maxsize=None)
def _ladder3_plain():
    """the plain lensed render of the three-level ladder: checked against the reference once, then the yardstick of the ladder modes"""
    want, st = _reference(None, BEHIND, 1, LADDER3)
    assert st["segment_hits"] >= MIN_HITS, st
    rp = _ctx(LADDER3, BEHIND)
    rp.set_uniforms(*_uniforms(None, 1, 1)); rp.render()
    _check(rp, want, "three-level ladder")
    out = rp.read_hdr().copy()
    rp.close()
    out.setflags(write=False)
    return out


def test_three_level_ladder():
    _ladder3_plain()
    want, st = _reference(None, BEHIND, 1, LADDER3)
    rc = _ctx(LADDER3, BEHIND, counters=True)                # the counting build: the same bits, the reference's counts
    rc.set_uniforms(*_uniforms(None, 1, 1)); rc.render()
    assert np.array_equal(_bits(rc.read_hdr()), _bits(_ladder3_plain()))
    _check_counters(rc, st, "three-level ladder")
    rc.close()


@pytest.mark.parametrize("mode", ["speculative", "superset", "temporal", "batches", "two_partitions"])
def test_ladder_modes_deliver_the_plain_lensed_bits(mode):
    want = _ladder3_plain()
    kw = {"speculative": dict(speculative_levels=2), "superset": dict(superset_levels=2), "temporal": dict(temporal=True),
          "batches": dict(frames_per_batch=4, frames_in_flight=4), "two_partitions": dict(devices=[0, 0], stripe_rows=9)}[mode]
    rp = _ctx(LADDER3, BEHIND, **kw)
    rp.set_uniforms(*_uniforms(None, 1, 1))
    for _ in range({"temporal": 3, "batches": 4}.get(mode, 1)):     # temporal: the third frame of a static sequence; batches: one full batch
        rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(want)), mode
    rp.close()


# ---- 4. several models
def test_one_inside_one_outside_one_invisible():
    models = ((3, (3.5, -1.5, -8.0), 1), (8, (-10.0, 0.0, 34.6), 1), (4, (-3.0, 1.0, -9.0), 0))    # inside R; beyond R; in front of the camera, invisible
    want, st = _reference(None, models, 1, ONE)
    assert st["segment_hits"] >= MIN_HITS, st
    bare = _reference(None, models[:1], 1, ONE)[0][-1]
    assert (_bits(bare) != _bits(want[-1])).any()                    # the model outside the sphere is in the picture too (the flat phase)
    rp = _ctx(ONE, models, counters=True)
    rp.set_uniforms(*_uniforms(None, 1, 3)); rp.render()
    _check(rp, want, "three models")
    _check_counters(rp, st, "three models")
    rp.close()


def test_coincident_copies_the_lower_index_wins():
    """Equal t on both: the strictly-nearer rule keeps slot 0's hit - the frame of slot 0 alone, bit for bit."""
    m = (3, (3.5, -1.5, -8.0), 1)
    want, st = _reference(None, (m, m), 1, ONE)
    assert st["segment_hits"] >= MIN_HITS, st
    assert np.array_equal(_bits(want[-1]), _bits(_reference(None, (m,), 1, ONE)[0][-1]))
    for method in (1, 0):
        one = _ctx(ONE, (m,)); one.set_uniforms(*_uniforms(None, method, 1)); one.render()
        two = _ctx(ONE, (m, m)); two.set_uniforms(*_uniforms(None, method, 2)); two.render()
        assert np.array_equal(_bits(one.read_hdr()), _bits(two.read_hdr())), method
        if method == 1:
            _check(two, want, "coincident copies")
        one.close(); two.close()


# ---- 5. a tree built on the device, the mesh moved into the sphere by vertex updates
def test_device_built_tree_moved_into_the_sphere():
    base = _model(7, (0.0, 0.0, 0.0)).arrays()
    rp = None
    hits = []
    for k, centre in enumerate(((0.5, 2.0, 31.0), (0.5, 2.0, 20.0), (0.5, 2.0, 11.0))):     # outside R = 20, straddling it, inside
        a = dict(base)
        a["points"] = base["points"].copy()
        a["points"][:, :3] += np.array(centre, np.float32)
        a = LB.with_tree(a, LB.build(a["points"], a["triangles"]))
        S = N.Scene(*_uniforms(None, 1, 1), *T.textures(), [a])
        st = {}
        want = LR.render_ladder_lensed(S, list(ONE), st)
        hits.append(st["segment_hits"])
        if rp is None:
            rp = _ctx(ONE, (a,), build=True, counters=True)
        else:
            rp.update_model_vertices(points=a["points"])
        rp.set_uniforms(*_uniforms(None, 1, 1)); rp.render()
        _check(rp, want, f"device-built tree, frame {k}")
        _check_counters(rp, st, f"device-built tree, frame {k}")
    rp.close()
    print("segment hits per frame", hits)
    assert hits[0] == 0 and hits[2] >= MIN_HITS, hits


# ---- 6. toggling on one ctx
def test_toggling_over_eight_frames_in_flight():
    models = SCENES["front_beside_the_hole"][1]
    pattern = [1, 0, 0, 1, 1, 0, 1, 0]
    single = {}
    for on in (0, 1):
        for k in (0, 1):                                             # two scene times, so that frames differ beyond the toggle
            rp = _ctx(ONE, models)                                    # every yardstick ctx has had the mode on ...
            rp.set_uniforms(*_uniforms(None, 1, 1, time=0.5 * k)); rp.render()
            if not on:                                               # ... and the off ones render again with it switched off
                rp.set_mesh_lensing(0); rp.render()
            single[(on, k)] = rp.read_hdr().copy()
            rp.close()
    assert (_bits(single[(0, 0)]) != _bits(single[(1, 0)])).any()
    never = B.RayPass(_cfg(ONE), device=0)                           # a ctx that never called the setter: the frame of one that switched the mode on and off again
    never.set_textures(*T.textures()); never.upload_model(_model(*models[0]), 0)
    never.set_uniforms(*_uniforms(None, 1, 1)); never.render()
    assert np.array_equal(_bits(never.read_hdr()), _bits(single[(0, 0)]))
    never.close()
    rp = _ctx(ONE, models, lensed=False, frames_in_flight=8)
    bufs = []
    for i, on in enumerate(pattern):
        rp.set_mesh_lensing(on)
        rp.set_uniforms(*_uniforms(None, 1, 1, time=0.5 * (i % 2)))
        bufs.append(T.DeviceBuffer(ONE[0][0] * ONE[0][1] * 16))
        rp.bind_output(bufs[-1].ptr.value, bufs[-1].nbytes)
        rp.render()
    rp.sync()
    for i, (on, b) in enumerate(zip(pattern, bufs)):
        assert np.array_equal(b.read(np.uint32), _bits(single[(on, i % 2)]).ravel()), (i, on)
        b.free()
    rp.close()


# ---- 7. the short traversal ring (restart trail) on segment rays
def test_short_traversal_ring():
    """libbhray_stack2.so (the same sources with a traversal ring of two entries): the segment traversals go through the restart trail"""
    import ctypes as C

    from bhusie_amd import _lib, layouts
    cam, models, _ = SCENES["behind_the_hole"]
    want, st = _reference(cam, tuple(models), 1, ONE)
    saved = _lib.lib()
    L = C.CDLL(T.variant_library("stack2"))
    layouts.declare(L)
    _lib._lib = L
    try:
        rp = _ctx(ONE, models, counters=True)
        rp.set_uniforms(*_uniforms(cam, 1, 1)); rp.render()
        _check(rp, want, "stack2")
        _check_counters(rp, st, "stack2")
        rp.close()
    finally:
        _lib._lib = saved


# ---- 8. refusals
@pytest.mark.parametrize("kw", [dict(literal=True), dict(eval_fma=True)], ids=["literal", "eval_fma"])
def test_refused_on_ctxs_of_the_other_evaluations(kw):
    rp = B.RayPass(_cfg(ONE), device=0, **kw)
    with pytest.raises(B.BhrayError) as e:
        rp.set_mesh_lensing(1)
    assert e.value.code == -5                                         # BHRAY_E_STATE
    rp.set_mesh_lensing(0)                                            # off is what such a ctx does anyway
    rp.close()


# ---- 9. fuzz
def test_fuzz_meshes_inside_the_sphere():
    """Eight seeded scenes in the manner of test_fuzz_mesh_scenes, the mesh centre drawn inside 0.8 R: both integrators, both host builders, an
    invisible mesh, the hole's disk turned at random."""
    rng = np.random.default_rng(11)
    tex = T.textures()
    total = 0
    for k in range(8):
        R = float(rng.uniform(12.0, 26.0))
        v = rng.normal(size=3); v /= np.linalg.norm(v)
        mpos = tuple(float(x) for x in v * rng.uniform(0.25, 0.8) * R)
        pos = rng.normal(size=3) * np.array([6.0, 3.0, 6.0]) + np.array([0.0, 0.0, -0.9 * R])
        fwd = np.array(mpos) * rng.uniform(0.3, 1.0) - pos; fwd = fwd / np.linalg.norm(fwd)
        cam = B.Camera(position=tuple(float(x) for x in pos), forward=tuple(float(x) for x in fwd), fov=float(rng.uniform(0.6, 1.6)))
        bh = B.BlackHole(relativity_sphere_radius=R, accretion_disk_rotation=tuple(float(x) for x in rng.uniform(-1, 1, size=3)))
        method = k % 2
        u = T.uniforms(camera=cam, black_hole=bh, integration_method=method, model_count=1, step_size=float(rng.uniform(0.1, 0.3)),
                       max_iterations=int(rng.integers(200, 700)))
        m = _model(int(rng.integers(2, 6)), mpos, 0 if k == 5 else 1, sah=(k % 4 == 3))
        st = {}
        want = LR.render_ladder_lensed(N.Scene(*u, *tex, [m.arrays()]), list(ONE), st)
        rp = _ctx(ONE, (m,), counters=True)
        rp.set_uniforms(*u); rp.render()
        _check(rp, want, f"fuzz case {k} (method {method}, mesh at {np.round(mpos, 1)}, R {R:.1f})")
        _check_counters(rp, st, f"fuzz case {k}")
        rp.close()
        print("fuzz case", k, st)
        if k == 5:
            assert st["segment_hits"] == 0
        total += st["segment_hits"]
    assert total >= 8 * MIN_HITS, total                                # the sweep does exercise the segment test
