"""-m gpu: mesh BVHs built on the GPU (bhray_upload_model_build / bhray_update_model_vertices).

 1. The tree read back from the device equals the NumPy restatement of §12 (tests/lbvh_ref.py) byte for byte once both are numbered
    breadth-first, on every mesh of the CPU list - the bench mesh spans all XCDs - and two builds give the same bytes.
 2. Frames traced through the device-built tree match the oracle run on the read-back tree to the project's parity bar, counters equal.
 3. read_model_bvh of a host-built slot returns the host tree.
 4. A vertex update gives the bytes (tree and frame) of a fresh upload of the moved mesh, in every frame mode.
 5. Mixed slots, Renderer.add_model(build="device"), partitioned ctxs, the display pass, bhray_render --bvh device.
 6. Errors are codes, and a refused upload leaves the slot as it was."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from bhusie_amd.model import NODE_DTYPE
from oracle import oracle as O
from tests import common as T
from tests import lbvh_ref as R
from tests import post_ref as PR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_CAPACITY = -1, -5, -8


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("lbvh_meshes")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _camera():
    d = np.array([-0.12, 0.0, 1.0]); d /= np.linalg.norm(d)
    return B.Camera(position=(0.0, 0.0, -40.0), forward=tuple(d), fov=1.2)       # the default model position (-10, 0, 30) fills much of the frame


def _ctx(cfg, tex, **kw):
    rp = B.RayPass(cfg, **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*tex)
    return rp


def _device_tree(rp, index=0):
    t = rp.read_model_bvh(index)
    return dict(nodes=R.renumber_bfs(t["nodes"]), bvh_lookup=t["bvh_lookup"], raw=t)


def _deformed(a, k):
    """geometry k of a mesh: 0 = as loaded; odd k = a seeded displacement of every point; even k > 0 = the whole mesh (points and normals) rotated"""
    pts, nrm = a["points"].copy(), a["normals"].copy()
    if k == 0:
        return pts, nrm
    if k % 2 == 1:
        h = assets._hash_u32(np.arange(pts.shape[0] * 3, dtype=np.uint32) * np.uint32(2654435761) ^ np.uint32(977 * k))
        pts[:, :3] += (0.6 * ((h & np.uint32(0xFFFF)).astype(np.float64) / 65535.0 - 0.5)).reshape(-1, 3).astype(np.float32)
        return pts, nrm
    ang = 0.4 * k
    rot = np.array([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]])
    pts[:, :3] = (pts[:, :3].astype(np.float64) @ rot.T).astype(np.float32)
    nrm[:, :3] = (nrm[:, :3].astype(np.float64) @ rot.T).astype(np.float32)
    return pts, nrm


# ---- 1. the tree ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_device_tree_equals_the_restatement_byte_for_byte(mesh_dir, name):
    a = R.case_arrays(name, mesh_dir)
    want = R.build(a["points"], a["triangles"])
    rp = _ctx(B.ladder_from_base((24, 14), 3, 2), T.textures())
    rp.upload_model_build(a)
    got = _device_tree(rp)
    info = rp.model_build_info()
    assert np.array_equal(got["bvh_lookup"], want["bvh_lookup"]), "sorted order"
    assert got["nodes"].shape == want["nodes"].shape
    assert got["nodes"].tobytes() == want["nodes"].tobytes(), "nodes (breadth-first numbering)"
    assert got["raw"]["nodes"][0]["obj_count"] > 0 or got["raw"]["nodes"][0]["left_child"] == 1      # root is node 0, its children follow it
    assert (info["built_on_device"], info["triangles"], info["nodes"], info["leaves"], info["max_leaf"], info["max_depth"]) == \
        (1, len(a["triangles"]), len(want["nodes"]), want["leaves"], want["max_leaf"], want["max_depth"])
    assert info["build_ms"] > 0.0 and info["upload_ms"] >= 0.0
    print(f"{name}: {info}")
    rp.upload_model_build(a)                                       # again, into the same slot: same bytes, device numbering included
    again = rp.read_model_bvh()
    assert again["nodes"].tobytes() == got["raw"]["nodes"].tobytes() and np.array_equal(again["bvh_lookup"], got["raw"]["bvh_lookup"])
    other = _ctx(B.ladder_from_base((24, 14), 3, 2), T.textures())
    other.upload_model_build(a, index=3)
    t3 = other.read_model_bvh(3)
    assert t3["nodes"].tobytes() == got["raw"]["nodes"].tobytes() and np.array_equal(t3["bvh_lookup"], got["raw"]["bvh_lookup"])
    rp.close(); other.close()


# ---- 2. parity -----------------------------------------------------------------------------------
def _parity(mesh_dir, method, what):
    tex = T.textures()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=method, model_count=1)
    cfg = B.ladder_from_base((40, 24), 3, 2)
    host = _ctx(cfg, tex)
    host.upload_model(B.load_model(str(mesh_dir / "sphere_24_32.obj")))
    host.set_uniforms(*u); host.render()
    ref_frame = host.read_hdr()
    host.close()
    rp = _ctx(cfg, tex, counters=True)
    rp.upload_model_build(a)
    rp.set_uniforms(*u); rp.render()
    got = rp.read_hdr()
    tree = rp.read_model_bvh()
    cnt = O.Counters()
    want = O.render_ladder(T.oracle_scene(*u, tex, [R.with_tree(a, tree)]), cfg.sizes(), cnt)
    T.assert_parity(got, want[-1], f"device-built tree vs oracle on the same tree, {what}")
    d = want[-1][..., 3] == 0
    assert np.array_equal(_bits(got[d]), _bits(want[-1][d])), what
    c = rp.counters()
    assert c == cnt.as_dict(), (what, c, cnt.as_dict())
    assert c["triangles"] > 0 and c["node_pairs"] > 0
    same = (_bits(got) == _bits(ref_frame)).all(axis=-1)
    print(f"{what}: pixels equal to the reference-tree frame bit for bit: {int(same.sum())} of {same.size} ({100.0 * same.mean():.3f} %)")
    rp.close()


@pytest.mark.parametrize("method", [1, 0])
@pytest.mark.parametrize("dense", ["0", "1"], ids=["latency", "dense"])
def test_device_tree_gives_the_oracles_frame(mesh_dir, monkeypatch, dense, method):
    monkeypatch.setenv("BHRAY_TRACE_DENSE", dense)
    _parity(mesh_dir, method, f"method {method}, BHRAY_TRACE_DENSE={dense}")


@pytest.fixture()
def stack2_library():
    """libbhray_stack2.so: the same sources with a traversal ring of two entries (the restart trail walks the device-built tree too)"""
    from bhusie_amd import _lib, layouts
    path = T.variant_library("stack2")
    saved = _lib.lib()
    L = C.CDLL(path)
    layouts.declare(L)
    _lib._lib = L
    yield
    _lib._lib = saved


@pytest.mark.parametrize("method", [1, 0])
def test_restart_trail_walks_the_device_tree(stack2_library, mesh_dir, method):
    _parity(mesh_dir, method, f"ring of 2, method {method}")


# ---- 3. any slot can be read back ----------------------------------------------------------------
def test_read_model_bvh_of_a_host_built_slot_returns_the_host_tree(mesh_dir):
    R.case_arrays("sphere_40_48", mesh_dir)
    model = B.load_model(str(mesh_dir / "sphere_40_48.obj"))
    rp = _ctx(B.ladder_from_base((24, 14), 3, 2), T.textures())
    for build in (model.build_bvh, model.build_bvh_sah):
        build()
        rp.upload_model(model, 2)
        a, t = model.arrays(), rp.read_model_bvh(2)
        assert R.renumber_bfs(t["nodes"]).tobytes() == R.renumber_bfs(a["nodes"]).tobytes()
        assert np.array_equal(t["bvh_lookup"], a["bvh_lookup"])
        info = rp.model_build_info(2)
        assert (info["built_on_device"], info["triangles"], info["nodes"]) == (0, len(a["triangles"]), len(a["nodes"]))
    rp.close()


# ---- 4. vertex updates ---------------------------------------------------------------------------
def _fresh(cfg, tex, a, pts, nrm, u):
    rp = _ctx(cfg, tex)
    rp.upload_model_build(dict(a, points=pts, normals=nrm))
    rp.set_uniforms(*u); rp.render()
    out = (rp.read_model_bvh(), rp.read_hdr().copy())
    rp.close()
    return out


def test_vertex_update_equals_a_fresh_upload(mesh_dir):
    tex = T.textures()
    a = R.case_arrays("ico4", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    cfg = B.ladder_from_base((40, 24), 3, 2)
    rp = _ctx(cfg, tex)
    rp.upload_model_build(a)
    rp.set_uniforms(*u); rp.render()
    frames = [rp.read_hdr().copy()]
    for k in (1, 2):
        pts, nrm = _deformed(a, k)
        rp.update_model_vertices(pts, nrm)
        rp.render()
        tree, frame = rp.read_model_bvh(), rp.read_hdr().copy()
        want_tree, want_frame = _fresh(cfg, tex, a, pts, nrm, u)
        assert tree["nodes"].tobytes() == want_tree["nodes"].tobytes() and np.array_equal(tree["bvh_lookup"], want_tree["bvh_lookup"]), k
        assert np.array_equal(_bits(frame), _bits(want_frame)), k
        ref = R.build(pts, a["triangles"])
        assert R.renumber_bfs(tree["nodes"]).tobytes() == ref["nodes"].tobytes(), k
        frames.append(frame)
    assert not np.array_equal(_bits(frames[0]), _bits(frames[1])) and not np.array_equal(_bits(frames[1]), _bits(frames[2]))   # the motion is in the picture
    pts, nrm = _deformed(a, 1)
    rp.update_model_vertices(points=pts)                           # one array only: the rotated normals stay
    rp.render()
    _, want_frame = _fresh(cfg, tex, a, pts, _deformed(a, 2)[1], u)
    assert np.array_equal(_bits(rp.read_hdr()), _bits(want_frame))
    rp.close()


def _animation(a, cfg, tex, bind=True, **kw):
    rp = _ctx(cfg, tex, **kw)
    rp.upload_model_build(a)
    w, h = cfg.frame_w, cfg.frame_h
    bufs, out = [], []
    for k in range(4):                                             # geometry 0 .. 3; with bound outputs nothing is read in between
        if k > 0:
            rp.update_model_vertices(*_deformed(a, k))
        rp.set_uniforms(*T.uniforms(camera=_camera(), integration_method=1, model_count=1, time=0.1 * k))
        if bind:
            bufs.append(T.DeviceBuffer(w * h * 16))
            rp.bind_output(bufs[-1].ptr.value, bufs[-1].nbytes)
            rp.render()
        else:
            rp.render()
            out.append(_bits(rp.read_hdr()).ravel().copy())
    if bind:
        rp.sync()
        out = [b.read(np.uint32) for b in bufs]
        for b in bufs:
            b.free()
    rp.close()
    return out


def test_frame_k_shows_geometry_k_in_every_frame_mode(mesh_dir):
    tex = T.textures()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    cfg = B.ladder_for_frame((200, 110), 3, 3)
    want = _animation(a, cfg, tex, bind=False, frames_in_flight=1)
    assert len({w.tobytes() for w in want}) == 4
    for kw in (dict(frames_in_flight=4), dict(frames_in_flight=2, frames_per_batch=3), dict(bind=False, temporal=True, frames_in_flight=1),
               dict(frames_in_flight=2, speculative_levels=2), dict(frames_in_flight=2, superset_levels=2)):
        got = _animation(a, cfg, tex, **kw)
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (kw, k)


# ---- 5. with the rest of the product -------------------------------------------------------------
def test_host_built_and_device_built_slots_side_by_side(mesh_dir):
    tex = T.textures()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    R.case_arrays("sphere_40_48", mesh_dir)
    host_model = B.load_model(str(mesh_dir / "sphere_40_48.obj"))
    host_model.set_transform((8.0, 2.0, 34.0), 1)
    cam = _camera()
    for method in (1, 0):
        u = T.uniforms(camera=cam, integration_method=method, model_count=2)
        cfg = B.ladder_from_base((40, 24), 3, 2)
        rp = _ctx(cfg, tex, counters=True)
        rp.upload_model(host_model, 0)
        rp.upload_model_build(a, 1)
        rp.set_uniforms(*u); rp.render()
        cnt = O.Counters()
        want = O.render_ladder(T.oracle_scene(*u, tex, [host_model.arrays(), R.with_tree(a, rp.read_model_bvh(1))]), cfg.sizes(), cnt)
        T.assert_parity(rp.read_hdr(), want[-1], f"mixed slots, method {method}")
        assert rp.counters() == cnt.as_dict()
        rp.close()


def _partitioned_equals_single(a, tex, cfg, u, **kw):
    one = _ctx(cfg, tex, frames_in_flight=1)
    one.upload_model_build(a)
    one.set_uniforms(*u); one.render()
    want = one.read_hdr().copy()
    one.close()
    rp = _ctx(cfg, tex, **kw)
    rp.upload_model_build(a)
    rp.set_uniforms(*u)
    for _ in range(3):
        rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(want)), kw
    pts, nrm = _deformed(a, 1)
    rp.update_model_vertices(pts, nrm)
    rp.render()
    moved = rp.read_hdr().copy()
    rp.close()
    one = _ctx(cfg, tex, frames_in_flight=1)
    one.upload_model_build(dict(a, points=pts, normals=nrm))
    one.set_uniforms(*u); one.render()
    assert np.array_equal(_bits(moved), _bits(one.read_hdr())), kw
    one.close()


def test_partitioned_ctx_gathers_the_single_ctx_frame(mesh_dir):
    tex = T.textures()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    cfg = B.ladder_for_frame((320, 180), 3, 3)
    _partitioned_equals_single(a, tex, cfg, u, devices=[0] * 8, stripe_rows=9, frames_per_batch=2, frames_in_flight=2)
    if B.lib().bhray_device_count() >= 2:
        _partitioned_equals_single(a, tex, cfg, u, devices=[0, 1], stripe_rows=9, frames_in_flight=2)


def test_renderer_add_model_on_the_device_and_the_display_pass(mesh_dir):
    tex = T.textures()
    R.case_arrays("sphere_24_32", mesh_dir)
    model = B.load_model(str(mesh_dir / "sphere_24_32.obj"))
    cfg = B.ladder_from_base((24, 14), 3, 3)                       # 208 x 118: no crop, wide enough for the bloom chain
    r = B.Renderer(cfg, device=0)
    r.ray_pass.set_textures(*tex)
    r.camera = _camera()
    r.ray_details.integration_method = 1
    assert r.add_model(model, build="device") == 0 and r.ray_details.model_count == 1
    assert r.ray_pass.model_build_info(0)["built_on_device"] == 1
    r.render()
    got = r.read_hdr()
    want = O.render_ladder(T.oracle_scene(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform(), tex,
                                          [R.with_tree(model.arrays(), r.ray_pass.read_model_bvh(0))]), cfg.sizes())[-1]
    T.assert_parity(got, want, "Renderer.add_model(build='device')")
    with pytest.raises(ValueError):
        r.add_model(model, build="gpu")
    r.ray_pass.resolve_display()
    img, sky = r.ray_pass.read_display(), r.ray_pass.read_sky()
    f, m = B.post_defaults()
    assert np.array_equal(img, PR.post_ref(sky, (np.float32(f.edge_threshold_min), np.float32(f.edge_threshold_max), int(f.iterations), np.float32(f.subpixel_quality)),
                                           np.float32(m.mix_ratio)))
    r.ray_pass.close()


def test_cpp_host_program_with_bvh_device(mesh_dir, tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    R.case_arrays("sphere_24_32", mesh_dir)
    obj = str(mesh_dir / "sphere_24_32.obj")
    outs = {}
    for flag in ("device", "reference"):
        out = tmp_path / f"{flag}.f32"
        r = subprocess.run([exe, str(out), "--rk", "--base", "24", "14", "--levels", "3", "--disk-size", "64", "--obj", obj, "--bvh", flag],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        w, h = (int(v) for v in r.stdout.strip().splitlines()[-1].split("x"))
        outs[flag] = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)      # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((24, 14), 3, 3), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.add_model(B.load_model(obj), build="device")
    r2.ray_details.integration_method = 1
    r2.render()
    assert np.array_equal(_bits(outs["device"]), _bits(r2.read_hdr()))
    bare = B.Renderer(B.ladder_from_base((24, 14), 3, 3), device=0)
    bare.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    bare.ray_details.integration_method = 1
    bare.render()
    assert not np.array_equal(_bits(outs["device"]), _bits(bare.read_hdr()))        # the mesh is in the picture
    assert outs["reference"].shape == outs["device"].shape          # --bvh reference is the default path
    r2.ray_pass.close(); bare.ray_pass.close()


# ---- 6. errors -----------------------------------------------------------------------------------
def test_errors_are_codes_and_a_refused_upload_keeps_the_slot(mesh_dir):
    tex = T.textures()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    rp = _ctx(B.ladder_from_base((40, 24), 3, 2), tex)
    rp.upload_model_build(a)
    rp.set_uniforms(*u); rp.render()
    before, tree = rp.read_hdr().copy(), rp.read_model_bvh()

    def code(call):
        with pytest.raises(B.BhrayError) as e:
            call()
        return e.value.code

    assert code(lambda: rp.upload_model_build(a, index=8)) == E_INVALID
    for col, bad in ((1, len(a["points"])), (0, -1), (4, len(a["normals"])), (5, -7)):
        tri = a["triangles"].copy()
        tri[len(tri) // 2, col] = bad
        assert code(lambda: rp.upload_model_build(dict(a, triangles=tri))) == E_INVALID, (col, bad)
    rp.render()                                                    # the slot is what it was
    assert np.array_equal(_bits(rp.read_hdr()), _bits(before))
    assert rp.read_model_bvh()["nodes"].tobytes() == tree["nodes"].tobytes()
    d = B.layouts.BhrayModelDesc()
    d.triangle_count = B.layouts.MAX_MODEL_VERTICES + 1
    assert rp._L.bhray_upload_model_build(rp._h, 0, C.byref(d)) == E_CAPACITY
    d.triangle_count, d.point_count = 1, B.layouts.MAX_MODEL_VERTICES + 1
    assert rp._L.bhray_upload_model_build(rp._h, 0, C.byref(d)) == E_CAPACITY
    pts, nrm = _deformed(a, 1)
    assert code(lambda: rp.update_model_vertices(pts[:-1], nrm)) == E_INVALID
    assert code(lambda: rp.update_model_vertices(pts, nrm[:-1])) == E_INVALID
    assert code(lambda: rp.update_model_vertices(pts, nrm, index=8)) == E_INVALID
    assert code(lambda: rp.update_model_vertices(pts, nrm, index=5)) == E_STATE            # empty slot
    R.case_arrays("sphere_40_48", mesh_dir)
    rp.upload_model(B.load_model(str(mesh_dir / "sphere_40_48.obj")), 1)
    assert code(lambda: rp.update_model_vertices(pts, nrm, index=1)) == E_STATE            # host-built slot
    assert code(lambda: rp.model_build_info(5)) == E_STATE and code(lambda: rp.read_model_bvh(5)) == E_STATE
    nn, nt = C.c_uint32(), C.c_uint32()
    small = np.zeros(4, dtype=NODE_DTYPE)
    assert rp._L.bhray_read_model_bvh(rp._h, 0, small.ctypes.data, 4, None, 0, C.byref(nn), C.byref(nt)) == E_INVALID
    assert (nn.value, nt.value) == (len(tree["nodes"]), len(a["triangles"]))               # caps too small: the counts are still written
    rp.upload_model_build(dict(a, triangles=a["triangles"][:0]))                           # 0 triangles: as bhray_upload_model, the slot is skipped
    rp.render()
    bare = _ctx(B.ladder_from_base((40, 24), 3, 2), tex)
    bare.set_uniforms(*T.uniforms(camera=_camera(), integration_method=1, model_count=0)); bare.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(bare.read_hdr()))
    rp.close(); bare.close()
