"""-m gpu: lensed meshes in ray batches, ray records and stills (bhray_set_mesh_lensing's BHRAY_LENS_RAYS).

  1. create_ray's rays under LENS_FRAMES | LENS_RAYS give the lensed `levels = 1` frame in every word (three scenes of tests/test_gpu_lensed.py, and the hole off the
     origin under a disk that reaches beyond the sphere), and tests/lensed_ref.py's frame at the project's bars; the lensed list differs from the flat-space list.
  2. 1 003 rays of arbitrary origin, results and records, against the restatement (tests/lensed_rays_ref.py): a mesh can be the first hit inside the sphere.
  3. n = 1, 63, 64, 65, 1 003: a ray does not depend on its batch (the lens phase's three triggers).
  4. The device form on a stream of the caller's, unusable records among the rays.          5. Trees built on the device; a pose moves a mesh.
  6. Stills: supersampled, one sample, lensing off, adaptive, a tent filter, an equirect camera, point stars - each against its existing restatement over the device's
     own lensed trace results.
  7. The rule: on = 1 refuses what it refused, on = 2 / 3 refuse the paths only; the other refusals; no visible model; frames keep their bits; an upload waits.
  8. Renderer.pick / render_records on the lensed mesh; ray_path raises.                     9. The C++ host: --lensed-mesh with --pick, --spp, --path.

The references run on the CPU once per process (tests/lensed_rays_ref.py: 23 s / 12 s for the 1 003-ray list, RK / Euler; the frames are test_gpu_lensed's, shared with
it); the GPU work of every test is milliseconds."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, cameras
from bhusie_amd.cameras import StillCamera
from bhusie_amd.renderer import StillFilter
from tests import accum_adaptive_ref as AD
from tests import accum_filter_ref as FR
from tests import accum_ref as A
from tests import accum_stars_ref as AS
from tests import common as T
from tests import lensed_rays_ref as LRR
from tests import ray_records_ref as RRR
from tests import test_gpu_lensed as GL
from tests.test_gpu_trace_rays import _Hip, _with_unusable_rays

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
ON = B.LENS_FRAMES | B.LENS_RAYS
EXACT = ("hit", "triangle", "iterations", "closest", "position")
FRONT = GL.SCENES["front_beside_the_hole"]
ONE = GL.ONE


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rec_words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _camera(cam):
    return B.Camera(position=cam[0], forward=cam[1], fov=cam[2]) if cam else B.Camera()


# ---- 1. pixel rays give the lensed frame -------------------------------------------------------------------
MIN_DIFFER = {"front_beside_the_hole": 14, "behind_the_hole": 31}      # pixels that differ from the flat-space ray list: the reference's counts with RK, the smaller of the two integrators'


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
@pytest.mark.parametrize("scene", ["front_beside_the_hole", "behind_the_hole", "camera_outside_straddling_R"])
def test_pixel_rays_give_the_lensed_frame(scene, method):
    cam, models, size = GL.SCENES[scene]
    models = tuple(models)
    (w, h), = size
    rays = cameras.pinhole_rays(_camera(cam), w, h)
    rp = GL._ctx(size, models, lensed=False)
    rp.set_uniforms(*GL._uniforms(cam, method, len(models)))
    rp.set_mesh_lensing(ON)
    got = rp.trace_rays(rays).reshape(h, w, 4)                     # without the feature: BHRAY_E_STATE here
    rp.render()
    frame = rp.read_hdr()
    assert np.isfinite(frame).all()
    differ = int((_bits(got) != _bits(frame)).sum())
    assert differ == 0, f"{scene} method {method}: {differ} of {frame.size} words differ from the lensed frame"
    want = GL._reference(cam, models, method, size)[0][-1]
    T.assert_parity(got, want, f"{scene} method {method}, the ray list against lensed_ref")
    d = want[..., 3] == 0
    assert np.array_equal(_bits(got[d]), _bits(want[d])), "direction pixels must be bit-identical"
    rp.set_mesh_lensing(0)
    flat = rp.trace_rays(rays).reshape(h, w, 4)
    changed = int((_bits(flat) != _bits(got)).any(axis=-1).sum())
    print(f"{scene} method {method}: {changed} pixels differ from the flat-space ray list")
    if scene in MIN_DIFFER:
        assert changed >= MIN_DIFFER[scene], (scene, changed)
    rp.close()


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_pixel_rays_with_the_hole_off_the_origin_under_a_wide_disk(method):
    """tests/test_gpu_trace_rays.py's HOLE_AWAY: the disk reaches beyond the sphere, so every disk hit has a defined colour - the frame is finite, and all of its words compare"""
    bh = B.BlackHole(position=(1.5, -0.75, 2.0), accretion_disk_outer=26.0)
    models = ((7, (2.0, 1.5, 13.0), 1),)                              # test_gpu_lensed's mesh behind the moved hole
    (w, h), = ONE
    u = T.uniforms(black_hole=bh, integration_method=method, model_count=1)
    rp = GL._ctx(ONE, models, lensed=False)
    rp.set_uniforms(*u)
    rp.set_mesh_lensing(ON)
    rp.render()
    frame = rp.read_hdr()
    assert np.isfinite(frame).all(), "the disk reaches beyond the sphere: no NaN pixel"
    got = rp.trace_rays(cameras.pinhole_rays(B.Camera(), w, h)).reshape(h, w, 4)
    assert int((_bits(got) != _bits(frame)).sum()) == 0
    rp.set_mesh_lensing(0)
    assert int((_bits(rp.trace_rays(cameras.pinhole_rays(B.Camera(), w, h)).reshape(h, w, 4)) != _bits(got)).any(axis=-1).sum()) >= 5, "the lensed mesh must be in the picture"
    rp.close()


# ---- 2. arbitrary rays, results and records ----------------------------------------------------------------
def _scene_ctx(method, build="host", lensing=ON):
    rp = B.RayPass(B.ladder_from_base((24, 14), 3, 1), device=0)
    rp.set_textures(*T.textures())
    for slot, m in enumerate(LRR.models()):
        (rp.upload_model_build if build == "device" else rp.upload_model)(m, slot)
    rp.set_uniforms(*LRR.uniforms(method))
    rp.set_mesh_lensing(lensing)
    return rp


@functools.lru_cache(maxsize=None)
def _gpu(method):
    """(ray pass, results, records) of rays(1003) under LENS_RAYS with host-built trees: computed once, left unchanged"""
    rp = _scene_ctx(method)
    out, rec = rp.trace_rays_records(LRR.rays())
    out.setflags(write=False); rec.setflags(write=False)
    return rp, out, rec


def _differ(got, want, field, keep):
    g, w = _bits(got[field]), _bits(want[field])
    d = (g != w) if g.ndim == 1 else (g != w).any(axis=1)
    return int(d[keep].sum())


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_arbitrary_rays_match_the_restatement(method):
    want_out, want, margin, seg_first, st = LRR.reference(method)
    c = LRR.conditions(method)
    print("method", method, "the reference's counts", c)
    LRR.assert_conditions(c, LRR.N_RAYS)                           # the floors, on the reference's own counts
    rp, out, rec = _gpu(method)
    n = want.shape[0]
    assert int((_bits(out) != _bits(rp.trace_rays(LRR.rays()))).sum()) == 0, "the results are not bhray_trace_rays' for the same rays"
    # results: tests/test_gpu_parity.py's bars
    alpha = int((out[:, 3] != want_out[:, 3]).sum())
    esc = want_out[:, 3] == 0.0
    dirs = int((_bits(out[esc]) != _bits(want_out[esc])).any(axis=1).sum())
    err = float(T.rel_err(out[~esc], want_out[~esc]).max(initial=0.0))
    # records: the exact words to the bit on every ray whose break test is not on its threshold; the transmittance within the bar, absolute
    keep = margin >= RRR.MARGIN_BAR
    differ = {f: _differ(rec, want, f, keep) for f in EXACT}
    terr = float(np.abs(rec["transmittance"][keep] - want["transmittance"][keep]).max(initial=0.0))
    print(f"method {method}: {alpha} alpha mismatches, {dirs} of {int(esc.sum())} escape directions differ, max rel colour err {err:.3g}; records that differ per field "
          f"{differ} of {int(keep.sum())} compared; max |transmittance error| {terr:.3g}; bit-identical records {100.0 * float((_rec_words(rec) == _rec_words(want)).all(axis=1).mean()):.2f} %")
    assert alpha == 0 and dirs == 0 and err <= T.REL_TOL, (alpha, dirs, err)
    assert int((~keep).sum()) <= RRR.MARGIN_SHARE * n
    for f in EXACT:
        assert differ[f] == 0, f"method {method}: {f} differs from the restatement on {differ[f]} rays"
    assert terr <= T.REL_TOL, terr
    assert (_rec_words(rec)[:, 3] >> 16 == 0).all(), "bits 16-31 of `hit` are zero"
    assert not (((rec["hit"] & 0xFF) == B.HIT_MESH) & (((rec["hit"] >> 8) & 0xFF) == 1)).any(), "a record names the invisible slot"


# ---- 3. a ray does not depend on its batch -----------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_a_ray_does_not_depend_on_its_batch(method):
    """n = 1 and 63: nobody marching is what runs the lens phase; 64 / 65: a second wave; 1 003: enough paused lanes, and the deferral count"""
    rp, full_out, full = _gpu(method)
    rays = LRR.rays()
    for n in (1, 63, 64, 65, LRR.N_RAYS):
        out, rec = rp.trace_rays_records(rays[:n])
        assert np.array_equal(_rec_words(rec), _rec_words(full[:n])), f"n = {n}: the records differ from the prefix of the whole list"
        assert np.array_equal(_bits(out), _bits(full_out[:n])), f"n = {n}: the results differ from the prefix of the whole list"
        assert np.array_equal(_bits(rp.trace_rays(rays[:n])), _bits(full_out[:n]))


# ---- 4. the device form ------------------------------------------------------------------------------------
def test_device_form_on_a_callers_stream_with_unusable_records():
    rays = LRR.rays()
    n = rays.shape[0]
    rp, host_out, host = _gpu(1)
    special, bad = _with_unusable_rays(rays)
    hip = _Hip()
    try:
        d_rays, d_out, d_rec, d_out2 = hip.alloc(n * 32), hip.alloc(n * 16), hip.alloc(n * 32 + 16), hip.alloc(n * 16)
        src = np.ascontiguousarray(special)
        assert hip.hip.hipMemcpyAsync(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D, hip.stream) == 0
        assert hip.hip.hipMemsetAsync(d_out, 0xFF, C.c_size_t(n * 16), hip.stream) == 0
        assert hip.hip.hipMemsetAsync(d_out2, 0xFF, C.c_size_t(n * 16), hip.stream) == 0
        assert hip.hip.hipMemsetAsync(d_rec, 0xFF, C.c_size_t(n * 32 + 16), hip.stream) == 0
        rp.trace_rays_records_device(d_rays.value, n, d_out.value, d_rec.value, stream=hip.stream.value)
        rp.trace_rays_device(d_rays.value, n, d_out2.value, stream=hip.stream.value)
        got = np.zeros((n, 4), dtype=np.float32)
        got2 = np.zeros((n, 4), dtype=np.float32)
        rec = np.zeros(n, dtype=B.RAY_RECORD_DTYPE)
        tail = np.zeros(4, dtype=np.uint32)
        assert hip.hip.hipMemcpyAsync(C.c_void_p(got.ctypes.data), d_out, C.c_size_t(got.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipMemcpyAsync(C.c_void_p(got2.ctypes.data), d_out2, C.c_size_t(got2.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipMemcpyAsync(C.c_void_p(rec.ctypes.data), d_rec, C.c_size_t(rec.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipMemcpyAsync(C.c_void_p(tail.ctypes.data), C.c_void_p(d_rec.value + n * 32), C.c_size_t(16), hip.D2H, hip.stream) == 0
        assert hip.hip.hipStreamSynchronize(hip.stream) == 0
        rp.sync()
        assert (tail == 0xFFFFFFFF).all(), "the kernel wrote behind record n - 1"
        unusable = [bad["nan_origin"], bad["inf_direction"], bad["zero_direction"]]
        for k in unusable:
            assert got[k].tolist() == [0.0, 0.0, 0.0, -1.0] and got2[k].tolist() == [0.0, 0.0, 0.0, -1.0], (k, got[k], got2[k])
            assert _rec_words(rec[k:k + 1])[0].tolist() == [0, 0, 0, B.HIT_UNUSABLE, 0xFFFFFFFF, 0, 0, 0], (k, rec[k])
        keep = np.ones(n, dtype=bool); keep[unusable] = False
        assert np.array_equal(_rec_words(rec[keep]), _rec_words(host[keep])), "the records differ from the host form's"
        assert np.array_equal(_bits(got[keep]), _bits(host_out[keep])) and np.array_equal(_bits(got2[keep]), _bits(host_out[keep]))
        assert (rec["hit"][bad["nan_pad"]] & 0xFF) != B.HIT_UNUSABLE, "the pad words are not looked at"
    finally:
        hip.close()


# ---- 5. trees built on the device --------------------------------------------------------------------------
def test_device_built_trees_and_a_pose():
    rp_host, host_out, host = _gpu(1)
    rp = _scene_ctx(1, build="device")
    trees = [rp.read_model_bvh(slot) for slot in range(len(LRR.SLOTS))]
    arrays = [m.arrays() for m in LRR.models()]
    assert any(not np.array_equal(t["bvh_lookup"], a["bvh_lookup"]) for t, a in zip(trees, arrays)), "the device's tree must be another tree than the host builder's"
    out, rec = rp.trace_rays_records(LRR.rays())
    assert np.array_equal(_bits(out), _bits(host_out)), "device-built trees give other results"
    assert np.array_equal(_rec_words(rec), _rec_words(host)), "the records under device-built trees do not name the caller's triangles"
    # slot 0 moved 40 up by a pose: the rays whose first hit it was answer differently
    aimed = ((host["hit"] & 0xFF) == B.HIT_MESH) & (((host["hit"] >> 8) & 0xFF) == 0)
    assert int(aimed.sum()) >= 30
    rp.set_model_pose([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 40.0, 0.0, 0.0, 1.0, 0.0], 0)
    moved_out, moved = rp.trace_rays_records(LRR.rays())
    changed = (_rec_words(moved) != _rec_words(host)).any(axis=1)
    print(f"{int(aimed.sum())} rays hit slot 0 first; {int((changed & aimed).sum())} of them changed with the pose, {int((changed & ~aimed).sum())} others")
    assert (changed & aimed).sum() == aimed.sum(), "a ray that hit slot 0 first must answer differently once the mesh is gone from there"
    rp.close()


# ---- 6. stills ---------------------------------------------------------------------------------------------
def _still_ctx(size=ONE, method=1, lensing=ON):
    rp = GL._ctx(size, tuple(FRONT[1]), lensed=False)
    rp.set_uniforms(*GL._uniforms(None, method, 1))
    rp.set_mesh_lensing(lensing)
    return rp


def _accumulate(rp, groups):
    rp.accum_begin()
    for g in groups:
        rp.accum_add(g)
    return rp.accum_read()


def _own_results(rp, S):
    """the device's own (lensed) trace results for the rays it generates itself for samples 0 .. S - 1 under the still camera in force"""
    return [rp.trace_rays(rp.accum_sample_rays(s)) for s in range(S)]


def _assert_words(got, want, what):
    differ = int((_bits(np.asarray(got).reshape(-1, 4)) != _bits(np.asarray(want).reshape(-1, 4))).sum())
    assert differ == 0, f"{what}: {differ} of {np.asarray(want).size} words differ from the restatement over the device's results"


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_supersampled_still(method):
    rp = _still_ctx(method=method)
    sky = T.textures()[2]
    per_sample = [rp.trace_rays(A.sample_rays(B.Camera(), rp.cfg, s)) for s in range(4)]
    want = A.mean(A.accumulate(per_sample, sky))
    got = _accumulate(rp, [4])
    _assert_words(got, want, f"accum_add(4), method {method}")
    _assert_words(_accumulate(rp, [1, 3]), want, "added as 1 + 3")
    # lensing off: the mesh inside the sphere leaves the still
    rp.set_mesh_lensing(0)
    off = _accumulate(rp, [4])
    assert int((_bits(off) != _bits(got)).any(axis=-1).sum()) >= 10, "the still with lensing off must differ from the lensed one"
    rp.close()


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_one_sample_is_the_resolved_lensed_frame(method):
    r = B.Renderer(GL._cfg(ONE), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = method
    r.add_model(GL._model(*FRONT[1][0]))
    r.mesh_lensing = True
    r.lens_ray_batches = True
    still = r.render_still(samples=1)
    r.render()
    frame = r.read_hdr()
    assert np.isfinite(frame).all()
    _assert_words(still, A.resolve(frame.reshape(-1, 4), T.textures()[2]), f"render_still(samples=1), method {method}")
    r.mesh_lensing = False
    assert int((_bits(r.render_still(samples=1)) != _bits(still)).any(axis=-1).sum()) >= 10
    r.ray_pass.close()


def test_adaptive_still():
    p = AD.Params(2, 8, 2, 0.05, 0.01)
    rp = _still_ctx()
    res = [rp.trace_rays(A.sample_rays(B.Camera(), rp.cfg, s)) for s in range(p.max_samples)]
    st = AD.State(res[0].shape[0])
    info, _ = AD.call(st, p, res, T.textures()[2])
    rp.accum_begin()
    got_info = rp.accum_add_adaptive(**p.as_kwargs())
    assert np.array_equal(rp.accum_read_counts().reshape(-1), st.issued)
    _assert_words(rp.accum_read(), AD.mean(st), "the adaptive mean")
    assert got_info == info
    assert len(np.unique(st.issued)) >= 2, "the frame must split into pixels that stop and pixels that go on"
    rp.close()


def test_tent_filtered_still():
    rp = _still_ctx()
    (w, h), = ONE
    want = A.mean(FR.accumulate(_own_results(rp, 4), T.textures()[2], FR.tent(1.5), w, h))
    rp.accum_set_filter(StillFilter.tent(1.5))
    _assert_words(_accumulate(rp, [4]), want, "the tent-filtered still")
    rp.close()


def test_equirect_still():
    size = ((32, 16),)
    rp = _still_ctx(size)
    rp.accum_set_camera(StillCamera.equirect())
    per_sample = _own_results(rp, 3)
    want = A.mean(A.accumulate(per_sample, T.textures()[2]))
    got = _accumulate(rp, [3])
    _assert_words(got, want, "the equirect still")
    rp.set_mesh_lensing(0)
    assert int((_bits(_accumulate(rp, [3])) != _bits(got)).any(axis=-1).sum()) >= 1, "the panorama must show the lensed mesh"
    rp.close()


def test_still_with_point_stars():
    cat = assets.star_catalogue(13, 7)
    rp = _still_ctx()
    (w, h), = ONE
    sky = T.textures()[2]
    per_sample = [r.reshape(h, w, 4) for r in _own_results(rp, 3)]
    want, _ = AS.mean([AS.starred(r, cat, None, sky, False)[0] for r in per_sample], sky, None)
    rp.set_stars(cat)
    rp.accum_set_stars(True)
    _assert_words(_accumulate(rp, [3]), want, "the still with point stars")
    rp.close()


# ---- 7. the rule -------------------------------------------------------------------------------------------
def test_the_rule():
    rays = LRR.rays()[:65]
    rp = _scene_ctx(1, lensing=0)
    off_out, off_rec = rp.trace_rays_records(rays)
    rp.accum_begin()
    calls = {"trace_rays": lambda: rp.trace_rays(rays), "trace_rays_records": lambda: rp.trace_rays_records(rays), "trace_rays_paths": lambda: rp.trace_rays_paths(rays, 0, 64),
             "accum_add": lambda: rp.accum_add(1), "accum_add_adaptive": lambda: rp.accum_add_adaptive(2, 4, 2, 0.05, 0.01)}
    rp.set_mesh_lensing(1)                                         # what `on != 0` has always meant: every batch is refused, with the message it had
    for name, call in calls.items():
        assert _code(call) == E_STATE, name
    with pytest.raises(B.BhrayError, match="ray batches under mesh lensing are not built"):
        rp.trace_rays(rays)
    rp.render()
    frame1 = rp.read_hdr().copy()
    lensed = {}
    for on in (3, 2):
        rp.set_mesh_lensing(on)
        for name, call in calls.items():
            if name == "trace_rays_paths":
                assert _code(call) == E_STATE, (on, name)
            elif name.startswith("accum_add"):
                rp.accum_begin(); call()
            else:
                call()
        lensed[on] = rp.trace_rays_records(rays)
        rp.render()
        assert np.array_equal(_bits(rp.read_hdr()), _bits(frame1)), f"a frame under on = {on} must have the bits of a frame under on = 1"
    assert np.array_equal(_bits(lensed[2][0]), _bits(lensed[3][0])) and np.array_equal(_rec_words(lensed[2][1]), _rec_words(lensed[3][1])), "on = 2 behaves as 3"
    assert np.array_equal(_rec_words(lensed[3][1]), _rec_words(_gpu(1)[2][:65]))
    assert not np.array_equal(_rec_words(lensed[3][1]), _rec_words(off_rec)), "the lensed records must differ from the flat-space ones"
    # `True` is 1, as before
    rp.set_mesh_lensing(True)
    assert _code(calls["trace_rays"]) == E_STATE
    # no visible model: every result and record has the bits it has with lensing off
    rp.set_mesh_lensing(0)
    for slot, (_, pos, _) in enumerate(LRR.SLOTS):
        rp.set_model_transform(pos, 0, index=slot)
    bare_out, bare_rec = rp.trace_rays_records(rays)
    rp.set_mesh_lensing(3)
    out, rec = rp.trace_rays_records(rays)
    assert np.array_equal(_bits(out), _bits(bare_out)) and np.array_equal(_rec_words(rec), _rec_words(bare_rec))
    assert not np.array_equal(_rec_words(bare_rec), _rec_words(off_rec)), "the visible models were in the flat-space records"
    rp.close()
    # the other refusals stay
    for kw in ({"literal": True}, {"eval_fma": True}):
        q = B.RayPass(GL._cfg(ONE), device=0, **kw)
        for on in (2, 3):
            assert _code(lambda: q.set_mesh_lensing(on)) == E_STATE, (kw, on)
        q.close()
    multi = GL._ctx(ONE, tuple(FRONT[1]), lensed=False, devices=[0, 0])
    multi.set_uniforms(*GL._uniforms(None, 1, 1))
    multi.set_mesh_lensing(3)
    assert _code(lambda: multi.trace_rays(rays)) == E_STATE and _code(lambda: multi.trace_rays_records(rays)) == E_STATE
    multi.close()
    fresh = GL._ctx(ONE, tuple(FRONT[1]), lensed=False)
    fresh.set_mesh_lensing(3)
    assert _code(lambda: fresh.trace_rays(rays)) == E_STATE          # before the first set_uniforms
    fresh.close()


def test_frames_keep_their_bits_and_an_upload_waits():
    rp = _still_ctx()
    rp.render()
    frame = rp.read_hdr().copy()
    alone = _accumulate(rp, [3])
    rp.render()
    batch = rp.trace_rays_records(LRR.rays()[:200])
    rp.accum_begin(); rp.accum_add(3)                               # behind a frame in flight
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed with lensed batches beside it"
    assert np.array_equal(_bits(rp.accum_read()), _bits(alone))
    # a model upload with lensed samples outstanding waits for them
    rp.accum_begin(); rp.accum_add(3)
    rp.upload_model(GL._model(3, (-4.0, 2.0, -7.0), 1), 0)
    assert np.array_equal(_bits(rp.accum_read()), _bits(alone)), "the outstanding lensed accumulation did not see the OLD model"
    assert int((_bits(_accumulate(rp, [3])) != _bits(alone)).any(axis=-1).sum()) >= 10, "the two models must differ in the image"
    again = rp.trace_rays_records(LRR.rays()[:200])
    assert not np.array_equal(_rec_words(again[1]), _rec_words(batch[1]))
    rp.sync()
    rp.close()


# ---- 8. picking --------------------------------------------------------------------------------------------
def _front_renderer(method):
    r = B.Renderer(GL._cfg(ONE), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = method
    r.add_model(GL._model(*FRONT[1][0]))
    return r


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_pick_names_the_lensed_mesh(method):
    (w, h), = ONE
    r = _front_renderer(method)
    for x, y in ((20, 5), (20, 6)):                                # with lensing off: the reference's answers are NONE / DISK
        assert r.pick(x, y)["hit"] in (B.HIT_NONE, B.HIT_DISK), (x, y)
    r.mesh_lensing = True
    with pytest.raises(B.BhrayError):                              # lens_ray_batches is off: the ctx's refusal, as before
        r.pick(20, 5)
    r.lens_ray_batches = True
    for x, y in ((20, 5), (20, 6)):
        p = r.pick(x, y)
        assert p["hit"] == B.HIT_MESH and p["model"] == 0 and 0 <= p["triangle"] < 80, (x, y, p)
    layers = r.render_records(cameras.pinhole_rays(r.camera, w, h), (h, w))
    mesh = (layers["hit"] & 0xFF) == B.HIT_MESH
    print(f"method {method}: {int(mesh.sum())} mesh pixels")
    assert int(mesh.sum()) >= 14 and mesh[5, 20] and mesh[6, 20]
    assert int(layers["triangle"][5, 20]) == r.pick(20, 5)["triangle"]
    img = r.render_rays(cameras.pinhole_rays(r.camera, w, h), (h, w))
    r.render()
    assert np.array_equal(_bits(img), _bits(r.read_hdr())), "render_rays of the pixel rays is the lensed frame"
    with pytest.raises(B.BhrayError) as e:
        r.ray_path(20, 5)
    assert e.value.code == E_STATE
    r.lens_ray_batches = False                                      # 3 -> 1 is a change of the setting, though both are true
    with pytest.raises(B.BhrayError):
        r.pick(20, 5)
    r.ray_pass.close()


# ---- 9. the C++ host ---------------------------------------------------------------------------------------
def test_cpp_host_under_lensed_mesh(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    radius, pos, _ = FRONT[1][0]
    lines = []
    GL._model(radius, pos)                                                             # (writes the mesh's OBJ file)
    home = B.load_model(os.path.join(GL._mesh_dir(), f"ico1_{radius}.obj")).arrays()["position"]      # a loaded model's own position: the reference's default, which bhray_render keeps
    for ln in assets.icosphere_mesh_obj(1, radius=float(radius)).splitlines():        # the mesh at its place in OBJ units (load_model scales by (0.5, -0.5, 0.5))
        if ln.startswith("v "):
            x, y, z = (float(v) for v in ln.split()[1:4])
            ln = "v %.6f %.6f %.6f" % (x + 2.0 * (pos[0] - float(home[0])), y - 2.0 * (pos[1] - float(home[1])), z + 2.0 * (pos[2] - float(home[2])))
        lines.append(ln)
    obj = tmp_path / "front.obj"
    obj.write_text("\n".join(lines) + "\n")
    out = tmp_path / "o.f32"
    base = [exe, str(out), "--rk", "--base", "32", "18", "--levels", "1", "--disk-size", "64", "--obj", str(obj), "--lensed-mesh"]
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)                          # bhray_render's textures
    r2 = B.Renderer(GL._cfg(ONE), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    r2.add_model(B.load_model(str(obj)))
    r2.mesh_lensing = True
    r2.lens_ray_batches = True
    want = r2.pick(20, 5)
    assert want["hit"] == B.HIT_MESH and want["model"] == 0
    r = subprocess.run(base + ["--pick", "20", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    assert f[:6] == ["pick", "20", "5", "hit=mesh", "model=0", f"triangle={want['triangle']}"], r.stdout
    assert int(dict(t.split("=") for t in f[3:] if "=" in t and t.count("=") == 1)["iterations"]) == want["iterations"]
    r = subprocess.run(base + ["--spp", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.float32).reshape(18, 32, 4)
    assert np.array_equal(_bits(got), _bits(r2.render_still(samples=4))), "the C++ host's lensed still differs from the Python host's"
    r = subprocess.run(base + ["--path", "20", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "lensed-mesh" in r.stderr
    r2.ray_pass.close()
