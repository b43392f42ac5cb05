"""-m gpu: ray records (bhray_trace_rays_records, bhray_trace_rays_records_device).

  1. The C oracle, no restatement in between: create_ray's rays of a 96 x 54 frame - closest approach and iterations are oracle.render_aux's channels 0 and 1 in every
     bit, the results are trace_rays' (both integrators; the default scene, the camera inside the sphere).
  2. 4 133 rays of arbitrary origin against the NumPy restatement (tests/ray_records_ref.py): hit, triangle, iterations, closest, position to the bit, the transmittance
     within 1e-4; rays whose break test sits on its threshold are left out.
  3. Meshes: two visible copies and an invisible one, half of the rays marching through the sphere first; model, triangle and position to the bit, for trees built on the
     host and on the device (the restatement fed the device's tree): the triangle indices are the caller's in both.
  4. n = 0, 1, 63, 64, 65.       5. The device variant on a stream of the caller's; unusable rays; a misaligned record array.
  6. Frames around a records batch keep their bits; the refused states; Renderer.pick / render_records; the C++ host's --pick."""
import ctypes as C
import functools

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras
from oracle import oracle as O
from tests import common as T
from tests import ray_records_ref as R
from tests import rays_ref as RR
from tests.test_gpu_trace_rays import _Hip, _with_unusable_rays

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
W, H = 96, 54
INSIDE = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)      # §15's camera inside the sphere
EXACT = ("hit", "triangle", "iterations", "closest", "position")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rec_words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)


def _ctx(cfg=None, **kw):
    rp = B.RayPass(cfg if cfg is not None else B.ladder_from_base((24, 14), 3, 1), **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*T.textures())
    return rp


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _differ(got, want, field, keep=None):
    g, w = _bits(got[field]), _bits(want[field])
    d = (g != w) if g.ndim == 1 else (g != w).any(axis=1)
    return int(d[keep].sum() if keep is not None else d.sum())


# ---- 1. the C oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("camera", ["default", "camera_inside_the_sphere"])
def test_closest_and_iterations_are_the_c_oracles(camera, method):
    cam = B.Camera() if camera == "default" else INSIDE
    u = T.uniforms(camera=cam, integration_method=method)
    aux = O.render_aux(T.oracle_scene(*u, T.textures()), (W, H))
    rays = cameras.pinhole_rays(cam, W, H)
    rp = _ctx()
    rp.set_uniforms(*u)
    out, rec = rp.trace_rays_records(rays)
    assert out.shape == (W * H, 4) and rec.shape == (W * H,) and rec.dtype == B.RAY_RECORD_DTYPE
    closest = int((_bits(rec["closest"].reshape(H, W)) != _bits(aux[..., 0])).sum())
    iters = int((rec["iterations"].reshape(H, W).astype(np.float32) != aux[..., 1]).sum())
    results = int((_bits(out) != _bits(rp.trace_rays(rays))).sum())
    print(f"{camera} method {method}: closest differs on {closest}, iterations on {iters} of {W * H} rays; {results} result words differ from trace_rays; kinds {R.kinds(rec)}")
    assert closest == 0, f"closest approach differs from oracle.render_aux on {closest} rays"
    assert iters == 0, f"iterations differ from oracle.render_aux on {iters} rays"
    assert results == 0, f"{results} result words differ from bhray_trace_rays'"
    k = R.kinds(rec)
    assert k["horizon"] > 0 and k["disk"] > 0 and k["none"] > 0 and k["mesh"] == 0


# ---- 2. arbitrary rays against the restatement ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_seeded(method):
    rp = _ctx()
    rp.set_uniforms(*RR.scene_uniforms(method))
    out, rec = rp.trace_rays_records(RR.seeded_rays())
    out.setflags(write=False); rec.setflags(write=False)
    return rp, out, rec


def _assert_records(got, want, margin, what):
    """the exact words to the bit on every ray whose break test is not on its threshold; the transmittance within the project's bar, absolute"""
    n = want.shape[0]
    keep = margin >= R.MARGIN_BAR
    assert int((~keep).sum()) <= R.MARGIN_SHARE * n
    differ = {f: _differ(got, want, f, keep) for f in EXACT}
    terr = float(np.abs(got["transmittance"][keep] - want["transmittance"][keep]).max(initial=0.0))
    same = float((_rec_words(got) == _rec_words(want)).all(axis=1).mean())
    print(f"{what}: rays that differ per field {differ} of {int(keep.sum())} compared ({n - int(keep.sum())} left out); max |transmittance error| {terr:.3g}; "
          f"bit-identical records {100.0 * same:.2f} %")
    for f in EXACT:
        assert differ[f] == 0, f"{what}: {f} differs from the restatement on {differ[f]} rays"
    assert terr <= T.REL_TOL, f"{what}: transmittance error {terr:.3g} > {T.REL_TOL}"


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_arbitrary_rays_match_the_restatement(method):
    want_out, want, margin, _ = R.seeded_reference(method)
    k = R.kinds(want)
    assert want.shape[0] == 4133 and min(k["none"], k["horizon"], k["disk"]) >= 300, k
    rp, out, rec = _gpu_seeded(method)
    assert int((_bits(out) != _bits(rp.trace_rays(RR.seeded_rays()))).sum()) == 0, "the results are not bhray_trace_rays' for the same rays"
    _assert_records(rec, want, margin, f"method {method}")
    assert (_rec_words(rec)[:, 3] >> 16 == 0).all(), "bits 16-31 of `hit` are zero"


# ---- 3. meshes ------------------------------------------------------------------------------------------
def _mesh_ctx(method, build):
    rp = _ctx()
    for slot, m in enumerate(R.mesh_models()):
        (rp.upload_model_build if build == "device" else rp.upload_model)(m, slot)
    rp.set_uniforms(*R.mesh_uniforms(method))
    return rp


def _assert_mesh(rp, want_all, what):
    want_out, want, margin, after_march = want_all
    c = R.mesh_conditions(want, after_march)
    print(what, c, R.kinds(want))
    assert c["mesh_slot0"] >= 150 and c["mesh_slot2"] >= 150 and c["after_march"] >= 50 and c["distinct_triangle_indices"] >= 30 and c["mesh_slot1"] == 0, c
    out, rec = rp.trace_rays_records(R.mesh_rays())
    assert int((_bits(out) != _bits(rp.trace_rays(R.mesh_rays()))).sum()) == 0
    _assert_records(rec, want, margin, what)
    assert not (((rec["hit"] & 0xFF) == B.HIT_MESH) & (((rec["hit"] >> 8) & 0xFF) == 1)).any(), "a record names the invisible slot"
    return rec


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_meshes_with_host_built_trees(method):
    _assert_mesh(_mesh_ctx(method, "host"), R.mesh_reference(method), f"host-built trees, method {method}")


def test_meshes_with_device_built_trees_name_the_callers_triangles():
    rp = _mesh_ctx(1, "device")
    trees = [rp.read_model_bvh(slot) for slot in (0, 1, 2)]
    host = [m.arrays() for m in R.mesh_models()]
    assert any(not np.array_equal(t["bvh_lookup"], h["bvh_lookup"]) for t, h in zip(trees, host)), "the device's tree must be another tree than the host builder's"
    rec = _assert_mesh(rp, R.mesh_trace(1, trees), "device-built trees")
    # the triangle indices refer to the caller's triangle array whichever tree found them: a ray whose first hit is a mesh under both trees names the same triangle
    # (two triangles hit at exactly the same t would be told apart by traversal order only; none is expected on this mesh, and at most a handful is tolerated: stated)
    ref = R.mesh_reference(1)[1]
    both = ((rec["hit"] & 0xFF) == B.HIT_MESH) & ((ref["hit"] & 0xFF) == B.HIT_MESH)
    other = int((rec["triangle"][both] != ref["triangle"][both]).sum())
    print(f"{int(both.sum())} rays hit a mesh first under both trees; {other} name another triangle")
    assert int(both.sum()) >= 300 and other == 0


# ---- 4. sizes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_a_rays_record_does_not_depend_on_its_batch(method):
    rays = RR.seeded_rays()
    rp, full_out, full = _gpu_seeded(method)
    for n in (0, 1, 63, 64, 65):
        out, rec = rp.trace_rays_records(rays[:n])
        assert out.shape == (n, 4) and rec.shape == (n,)
        assert np.array_equal(_rec_words(rec), _rec_words(full[:n])), f"n = {n}: the records differ from the prefix of the full batch"
        assert np.array_equal(_bits(out), _bits(full_out[:n]))
    # the results may be left out (a NULL out_rgba32f)
    recs = np.zeros(65, dtype=B.RAY_RECORD_DTYPE)
    src = np.ascontiguousarray(rays[:65])
    rc = B.lib().bhray_trace_rays_records(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), 65, None, recs.ctypes.data_as(C.POINTER(B.BhrayRayRecord)))
    assert rc == 0 and np.array_equal(_rec_words(recs), _rec_words(full[:65]))
    assert B.lib().bhray_trace_rays_records(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), 65, None, None) == E_INVALID


# ---- 5. the device variant ------------------------------------------------------------------------------
def test_device_variant_on_a_callers_stream_and_unusable_records():
    rays = RR.seeded_rays()
    n = rays.shape[0]
    rp, host_out, host = _gpu_seeded(1)
    special, bad = _with_unusable_rays(rays)
    hip = _Hip()
    try:
        d_rays, d_out, d_rec = hip.alloc(n * 32), hip.alloc(n * 16), hip.alloc(n * 32 + 16)
        src = np.ascontiguousarray(special)
        assert hip.hip.hipMemcpyAsync(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D, hip.stream) == 0
        assert hip.hip.hipMemsetAsync(d_out, 0xFF, C.c_size_t(n * 16), hip.stream) == 0
        assert hip.hip.hipMemsetAsync(d_rec, 0xFF, C.c_size_t(n * 32 + 16), hip.stream) == 0
        rp.trace_rays_records_device(d_rays.value, n, d_out.value, d_rec.value, stream=hip.stream.value)
        got = np.zeros((n, 4), dtype=np.float32)
        rec = np.zeros(n, dtype=B.RAY_RECORD_DTYPE)
        tail = np.zeros(4, dtype=np.uint32)
        assert hip.hip.hipMemcpyAsync(C.c_void_p(got.ctypes.data), d_out, C.c_size_t(got.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipMemcpyAsync(C.c_void_p(rec.ctypes.data), d_rec, C.c_size_t(rec.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipMemcpyAsync(C.c_void_p(tail.ctypes.data), C.c_void_p(d_rec.value + n * 32), C.c_size_t(16), hip.D2H, hip.stream) == 0
        assert hip.hip.hipStreamSynchronize(hip.stream) == 0
        rp.sync()
        assert (tail == 0xFFFFFFFF).all(), "the kernel wrote behind record n - 1"
        unusable = [bad["nan_origin"], bad["inf_direction"], bad["zero_direction"]]
        for k in unusable:
            assert got[k].tolist() == [0.0, 0.0, 0.0, -1.0], (k, got[k])
            assert _rec_words(rec[k:k + 1])[0].tolist() == [0, 0, 0, B.HIT_UNUSABLE, 0xFFFFFFFF, 0, 0, 0], (k, rec[k])
        keep = np.ones(n, dtype=bool); keep[unusable] = False
        assert np.array_equal(_rec_words(rec[keep]), _rec_words(host[keep])), "the records differ from the host variant's"
        assert np.array_equal(_bits(got[keep]), _bits(host_out[keep]))
        assert (rec["hit"][bad["nan_pad"]] & 0xFF) != B.HIT_UNUSABLE, "the pad words are not looked at"
        # the host variant refuses the same list as a whole and leaves both outputs alone
        out = np.full((n, 4), 7.0, dtype=np.float32)
        recs = np.zeros(n, dtype=B.RAY_RECORD_DTYPE); recs["iterations"] = 77
        rc = B.lib().bhray_trace_rays_records(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), n, out.ctypes.data_as(C.POINTER(C.c_float)),
                                              recs.ctypes.data_as(C.POINTER(B.BhrayRayRecord)))
        assert rc == E_INVALID and (out == 7.0).all() and (recs["iterations"] == 77).all()
        # a misaligned or missing record array, n == 0, n beyond the limit
        assert _code(lambda: rp.trace_rays_records_device(d_rays.value, 5, d_out.value, d_rec.value + 4)) == E_INVALID
        assert _code(lambda: rp.trace_rays_records_device(d_rays.value, 5, d_out.value, d_rec.value + 8)) == E_INVALID
        assert _code(lambda: rp.trace_rays_records_device(d_rays.value, 5, d_out.value, 0)) == E_INVALID
        assert _code(lambda: rp.trace_rays_records_device(d_rays.value, (1 << 26) + 1, d_out.value, d_rec.value)) == E_INVALID
        rp.trace_rays_records_device(d_rays.value, 0, d_out.value, d_rec.value, stream=hip.stream.value)
        rp.sync()
    finally:
        hip.close()


# ---- 6. state, and the hosts ----------------------------------------------------------------------------
def test_frames_before_and_after_a_records_batch_keep_their_bits():
    cfg = B.ladder_from_base((40, 24), 3, 2)
    cams = [B.Camera(position=(0.0, 0.0, -19.0)), B.Camera(position=(1.0, 0.5, -30.0), forward=(0.0, 0.05, 1.0))]

    def run(with_batch):
        rp = _ctx(cfg, frames_in_flight=4)
        first = B.PinnedFrame(len(rp.local_rows()), rp.frame_size[0])
        rp.set_uniforms(*T.uniforms(camera=cams[0], integration_method=1))
        rp.render()
        ticket = rp.read_hdr_async(first)
        batch = rp.trace_rays_records(RR.seeded_rays()[:1000])[1] if with_batch else None
        rp.set_uniforms(*T.uniforms(camera=cams[1], integration_method=1))
        rp.render()
        second = rp.read_hdr().copy()
        rp.wait_read(ticket)
        frames = [first.array.copy(), second]
        first.free()
        return frames, batch

    plain, _ = run(False)
    mixed, batch = run(True)
    for k in range(2):
        assert np.array_equal(_bits(plain[k]), _bits(mixed[k])), f"frame {k} changed with a records batch between the renders"
    assert np.array_equal(_rec_words(batch), _rec_words(_gpu_seeded(1)[2][:1000])), "the batch between two frames differs from the batch alone"


def test_refused_states_are_those_of_trace_rays():
    rays = RR.seeded_rays()[:65]
    u = RR.scene_uniforms(1)
    rp = _ctx()
    assert _code(lambda: rp.trace_rays_records(rays)) == E_STATE           # before the first set_uniforms
    rp.set_uniforms(*u)
    good = rp.trace_rays_records(rays)[1]
    for kw in ({"literal": True}, {"eval_fma": True}):
        q = _ctx(**kw)
        q.set_uniforms(*u)
        assert _code(lambda: q.trace_rays_records(rays)) == E_STATE, kw
    rp.set_mesh_lensing(True)
    assert _code(lambda: rp.trace_rays_records(rays)) == E_STATE
    rp.set_mesh_lensing(False)
    assert np.array_equal(_rec_words(rp.trace_rays_records(rays)[1]), _rec_words(good))
    multi = _ctx(devices=[0, 0])
    multi.set_uniforms(*u)
    assert _code(lambda: multi.trace_rays_records(rays)) == E_STATE
    assert _code(lambda: rp.trace_rays_records(np.full((1, 6), np.nan, np.float32))) == E_INVALID
    counting = _ctx(counters=True)                                         # the kernels that do not count: its counters do not move
    counting.set_uniforms(*u)
    counting.render(); counting.sync()
    before = counting.counters()
    assert np.array_equal(_rec_words(counting.trace_rays_records(rays)[1]), _rec_words(good))
    assert counting.counters() == before


MESH_CAM = B.Camera(position=(0.0, 0.0, -60.0), forward=(-0.1, 0.0, 1.0), fov=1.0)
MESH_AT = (-22.0, 4.0, -25.0)               # §15's mesh in flat space, in front of MESH_CAM


def test_pick_and_render_records():
    r = B.Renderer(B.ladder_from_base((W, H), 3, 1), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    assert r.pick(W // 2, H // 2)["hit"] == B.HIT_HORIZON, "the default scene's centre pixel looks into the hole"
    # a mesh in slot 1 (slot 0 holds a copy behind the camera): the frame shows it, pick names its slot
    r.camera = MESH_CAM
    r.add_model(RR.mesh_model((0.0, 0.0, -120.0)))
    slot = r.add_model(RR.mesh_model(MESH_AT))
    assert slot == 1
    r.render()
    with_mesh = r.read_hdr()
    r.ray_pass.set_model_transform(MESH_AT, 0, index=1)
    r.render()
    without = r.read_hdr()
    r.ray_pass.set_model_transform(MESH_AT, 1, index=1)
    ys, xs = np.nonzero((_bits(with_mesh) != _bits(without)).any(axis=2))
    assert ys.size >= 50, "the frame must show the mesh"
    layers = r.render_records(cameras.pinhole_rays(MESH_CAM, W, H), (H, W))
    assert layers.shape == (H, W) and layers.dtype == B.RAY_RECORD_DTYPE
    for k in (0, ys.size // 2, ys.size - 1):
        x, y = int(xs[k]), int(ys[k])
        p = r.pick(x, y)
        assert p["hit"] == B.HIT_MESH and p["model"] == 1, (x, y, p)
        assert 0 <= p["triangle"] < r.models[1].arrays()["triangles"].shape[0]
        assert np.array_equal(_rec_words(layers[y:y + 1, x]), _rec_words(r.ray_pass.trace_rays_records(cameras.pinhole_rays(MESH_CAM, W, H, pixel=(x, y)))[1]))
        assert p["triangle"] == int(layers["triangle"][y, x]) and p["iterations"] == int(layers["iterations"][y, x])
    p = r.pick(W - 1, 0)
    assert p["hit"] in (B.HIT_NONE, B.HIT_DISK, B.HIT_HORIZON) and p["model"] is None and p["triangle"] == -1
    with pytest.raises(ValueError):
        r.pick(W, 0)
    # rays that are not traced (a fisheye's pixels outside its circle): the device form's answer
    fr = cameras.fisheye_rays(MESH_CAM.position, MESH_CAM.forward, 33, 33, 3.0)
    fl = r.render_records(fr, (33, 33))
    outside = (fr[:, 4:7] == 0.0).all(axis=1).reshape(33, 33)
    assert outside[0, 0] and not outside[16, 16]
    assert (_rec_words(fl[outside]) == np.array([0, 0, 0, B.HIT_UNUSABLE, 0xFFFFFFFF, 0, 0, 0], np.uint32)).all()
    assert ((fl["hit"][~outside] & 0xFF) != B.HIT_UNUSABLE).all()


def test_cpp_host_prints_a_pick(tmp_path):
    """bhray_render --pick X Y: the frame's file as without it, and one line with the record of that pixel - what Renderer.pick says about the same pixel of the same scene
    (the two hosts form the ray with the same binary32 arithmetic)"""
    import os
    import subprocess
    from bhusie_amd import assets
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "frame.f32"
    base = [exe, str(out), "--rk", "--base", "24", "14", "--levels", "1", "--disk-size", "64"]
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)                                # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((24, 14), 3, 1), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    names = {B.HIT_NONE: "none", B.HIT_HORIZON: "horizon", B.HIT_DISK: "disk", B.HIT_MESH: "mesh"}
    seen = set()
    for x, y in ((12, 7), (12, 1), (0, 0)):
        r = subprocess.run(base + ["--pick", str(x), str(y)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        assert lines[-2] == "24x14" and np.fromfile(out, dtype=np.float32).size == 24 * 14 * 4
        f = lines[-1].split()
        want = r2.pick(x, y)
        print(lines[-1], want)
        assert f[:3] == ["pick", str(x), str(y)] and f[3] == "hit=" + names[want["hit"]] and f[4] == "model=-1" and f[5] == "triangle=-1", lines[-1]
        field = {t.split("=")[0]: t.split("=")[1] for t in f[3:] if "=" in t}
        assert int(field["iterations"]) == want["iterations"]
        assert abs(float(field["closest"]) - want["closest"]) <= 1e-5 * want["closest"] and abs(float(field["transmittance"]) - want["transmittance"]) <= 1e-5
        seen.add(want["hit"])
    assert len(seen) >= 2, "the three pixels must not all end alike"
    far = subprocess.run(base + ["--pick", "99", "7"], capture_output=True, text=True, timeout=120)
    assert far.returncode == 1 and "outside the frame" in far.stderr
