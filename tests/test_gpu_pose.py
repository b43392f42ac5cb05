"""-m gpu: device-built meshes posed on the GPU (bhray_set_model_pose, bhray_update_model_vertices_device, bhray_read_model_vertices).

  1. The pose kernel against the restatement (tests/pose_ref.py) byte for byte, at the sizes where a 256-thread launch over points + normals can go wrong.
  2. Tree and frame of a posed slot = those of a fresh upload / a host vertex update of the restatement's arrays, and the tree of tests/lbvh_ref.py.
  3. The pose is absolute; None restores the rest arrays.           4. Vertex updates of a posed slot replace the REST arrays.
  5. Vertex data from device memory, behind a stream.                6. Frame k shows pose k in every frame mode.
  7. Partitioned ctxs.   8. Lensed meshes.   9. Errors keep the slot.   10. Renderer / bhray_render --pose.   11. Build info."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from tests import common as T
from tests import lbvh_ref as R
from tests import pose_ref as PR
from tests import post_ref as PO

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
SMALL = ((40, 24), 3, 2)


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pose_meshes")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _camera():
    d = np.array([-0.12, 0.0, 1.0]); d /= np.linalg.norm(d)
    return B.Camera(position=(0.0, 0.0, -40.0), forward=tuple(d), fov=1.2)       # the default model position (-10, 0, 30) fills much of the frame


def _ctx(cfg, tex, **kw):
    rp = B.RayPass(cfg, **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*tex)
    return rp


def _small():
    return B.ladder_from_base(*SMALL)


def _pose(k):
    """pose k of the animations (k >= 1): a turn about a point off the mesh's centre, scaled a little; all keep the mesh in the picture"""
    return PR.from_euler((0.3 * k, 0.7 - 0.25 * k, -0.2 * k), (1.0, -0.5, 0.5), 1.0 + 0.05 * k)


def _posed(a, m):
    p, n = PR.apply(a["points"], a["normals"], m)
    return dict(a, points=p, normals=n)


def _same_tree(t, u):
    return t["nodes"].tobytes() == u["nodes"].tobytes() and np.array_equal(t["bvh_lookup"], u["bvh_lookup"])


def _same_vertices(v, a):
    return np.array_equal(_bits(v["points"]), _bits(a["points"])) and np.array_equal(_bits(v["normals"]), _bits(a["normals"]))


def _state(rp):
    """(vertices, tree, frame) of slot 0 after one more render"""
    rp.render()
    return rp.read_model_vertices(), rp.read_model_bvh(), rp.read_hdr().copy()


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


# ---- 1. the kernel ---------------------------------------------------------------------------------
def _fan(point_count, normal_count, seed):
    """a triangle fan over point_count points with normal_count normals: w lanes of arbitrary bits, some -0 coordinates"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-6.0, 6.0, (point_count, 4)).astype(np.float32)
    nrm = rng.uniform(-1.0, 1.0, (normal_count, 4)).astype(np.float32)
    for arr in (pts, nrm):
        w = rng.integers(0, 2 ** 32, len(arr), dtype=np.uint64).astype(np.uint32)
        w[0] = 0x7FC12345                                          # a NaN with a payload
        _bits(arr)[:, 3] = w
        for i in range(0, len(arr), 5):
            _bits(arr)[i, (i // 5) % 3] = 0x80000000               # -0
    T_ = point_count - 2
    i = np.arange(1, T_ + 1)
    tri = np.zeros((T_, 6), dtype=np.int32)
    tri[:, 0], tri[:, 1], tri[:, 2] = 0, i, i + 1
    for c in range(3):
        tri[:, 3 + c] = (7 * i + 3 * c) % normal_count
    return dict(position=np.array((-10.0, 0.0, 30.0), np.float32), visible=1, points=pts, normals=nrm, triangles=tri)


KERNEL_POSES = {
    "identity": PR.IDENTITY,
    "rigid": PR.from_euler((0.4, -1.1, 2.3), (3.0, -2.0, 1.5), 1.0),
    "scaled": PR.from_euler((-0.9, 0.2, 0.6), (0.0, 0.0, 0.0), 1.5),
    "shear": np.array([[1.0, 0.35, -0.2, 0.75], [0.0, 0.8, 0.5, -1.25], [0.1, 0.0, 1.3, 2.0]], dtype=np.float32),
    "collapse": np.array([[0.0, 0.0, 0.0, 1.5], [0.0, 0.0, 0.0, -2.5], [0.0, 0.0, 0.0, 0.25]], dtype=np.float32),
}


@pytest.mark.parametrize("point_count", [3, 63, 64, 65, 255, 256, 257, 1025])
def test_pose_kernel_equals_the_restatement_byte_for_byte(point_count):
    rp = _ctx(B.ladder_from_base((24, 14), 3, 2), T.textures())
    for normal_count in (1, 64, 257):                              # independent of point_count (an OBJ mesh's counts differ)
        a = _fan(point_count, normal_count, 100 * point_count + normal_count)
        rp.upload_model_build(a)
        for name, m in KERNEL_POSES.items():
            rp.set_model_pose(m)
            want = _posed(a, m)
            got = rp.read_model_vertices()
            what = (point_count, normal_count, name)
            assert got["points"].shape == want["points"].shape and got["normals"].shape == want["normals"].shape, what
            assert np.array_equal(_bits(got["points"]), _bits(want["points"])), what
            assert np.array_equal(_bits(got["normals"]), _bits(want["normals"])), what
            ref = R.build(want["points"], a["triangles"])           # "collapse": every point coincides, the tree is still the restatement's
            tree = rp.read_model_bvh()
            assert R.renumber_bfs(tree["nodes"]).tobytes() == ref["nodes"].tobytes() and np.array_equal(tree["bvh_lookup"], ref["bvh_lookup"]), what
        if name == "collapse":
            assert len(np.unique(_bits(got["points"])[:, :3], axis=0)) == 1
        rp.set_model_pose(None)
        assert _same_vertices(rp.read_model_vertices(), a), (point_count, normal_count, "rest")
    rp.close()


# ---- 2. tree and frame -----------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 0])
@pytest.mark.parametrize("name", ["ico4", "sphere_24_32"])
def test_posed_slot_equals_a_fresh_upload_and_a_host_update(mesh_dir, name, method):
    tex, cfg = T.textures(), _small()
    a = R.case_arrays(name, mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=method, model_count=1)
    m = _pose(1)
    want = _posed(a, m)
    rp = _ctx(cfg, tex)
    rp.upload_model_build(a)
    rp.set_uniforms(*u)
    rp.set_model_pose(m)
    verts, tree, frame = _state(rp)
    rp.close()
    assert _same_vertices(verts, want)
    fresh = _ctx(cfg, tex)
    fresh.upload_model_build(want)
    fresh.set_uniforms(*u)
    _, tree1, frame1 = _state(fresh)
    fresh.close()
    assert _same_tree(tree, tree1) and np.array_equal(_bits(frame), _bits(frame1))
    upd = _ctx(cfg, tex)
    upd.upload_model_build(a)
    upd.set_uniforms(*u)
    upd.update_model_vertices(want["points"], want["normals"])
    _, tree2, frame2 = _state(upd)
    upd.close()
    assert _same_tree(tree, tree2) and np.array_equal(_bits(frame), _bits(frame2))
    ref = R.build(want["points"], a["triangles"])
    assert R.renumber_bfs(tree["nodes"]).tobytes() == ref["nodes"].tobytes() and np.array_equal(tree["bvh_lookup"], ref["bvh_lookup"])


# ---- 3. absolute; None restores --------------------------------------------------------------------
def test_pose_is_absolute_and_none_restores_the_rest_arrays(mesh_dir):
    tex, cfg = T.textures(), _small()
    a = R.case_arrays("ico4", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    never = _ctx(cfg, tex)
    never.upload_model_build(a); never.set_uniforms(*u)
    rest = _state(never)
    never.close()
    only_b = _ctx(cfg, tex)
    only_b.upload_model_build(a); only_b.set_uniforms(*u)
    only_b.set_model_pose(_pose(2))
    b_alone = _state(only_b)
    only_b.close()
    rp = _ctx(cfg, tex)
    rp.upload_model_build(a); rp.set_uniforms(*u)
    assert _same_vertices(rp.read_model_vertices(), a)
    rp.set_model_pose(_pose(1))
    after_a = _state(rp)
    rp.set_model_pose(_pose(2))
    after_b = _state(rp)
    rp.set_model_pose(None)
    back = _state(rp)
    rp.set_model_pose(None)                                        # again, and on a slot whose pose is already off
    back2 = _state(rp)
    rp.close()
    for got, want, what in ((after_b, b_alone, "A then B = B"), (back, rest, "None = never posed"), (back2, rest, "None twice")):
        assert _same_vertices(got[0], want[0]) and _same_tree(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2])), what
    assert _same_vertices(after_a[0], _posed(a, _pose(1)))
    frames = [_bits(s[2]).tobytes() for s in (rest, after_a, after_b)]
    assert len(set(frames)) == 3                                   # the motion is in the picture


# ---- 4. rest replacement ---------------------------------------------------------------------------
def _other_geometry(a):
    """another mesh of the same counts and triangles: every point displaced by a seeded amount, the normals turned"""
    pts, nrm = a["points"].copy(), a["normals"].copy()
    h = assets._hash_u32(np.arange(pts.shape[0] * 3, dtype=np.uint32) * np.uint32(2654435761) ^ np.uint32(977))
    pts[:, :3] += (0.6 * ((h & np.uint32(0xFFFF)).astype(np.float64) / 65535.0 - 0.5)).reshape(-1, 3).astype(np.float32)
    nrm[:, :3] = nrm[:, [2, 0, 1]]
    return pts, nrm


def test_vertex_update_of_a_posed_slot_replaces_the_rest_arrays(mesh_dir):
    tex, cfg = T.textures(), _small()
    a = R.case_arrays("ico4", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    m = _pose(1)
    pts, nrm = _other_geometry(a)

    def fresh(arrays):
        f = _ctx(cfg, tex)
        f.upload_model_build(arrays); f.set_uniforms(*u)
        out = _state(f)
        f.close()
        return out

    rp = _ctx(cfg, tex)
    rp.upload_model_build(a); rp.set_uniforms(*u)
    rp.set_model_pose(m)
    rp.update_model_vertices(pts, nrm)
    got = _state(rp)
    want = _posed(dict(a, points=pts, normals=nrm), m)
    f = fresh(want)
    assert _same_vertices(got[0], want) and _same_tree(got[1], f[1]) and np.array_equal(_bits(got[2]), _bits(f[2]))
    rp.update_model_vertices(points=a["points"])                   # one array: the other REST array (the new normals) stays
    got = _state(rp)
    want = _posed(dict(a, normals=nrm), m)
    f = fresh(want)
    assert _same_vertices(got[0], want) and _same_tree(got[1], f[1]) and np.array_equal(_bits(got[2]), _bits(f[2]))
    rp.update_model_vertices(normals=a["normals"])
    assert _same_vertices(rp.read_model_vertices(), _posed(a, m))
    rp.set_model_pose(None)                                        # the rest arrays are what the updates left
    assert _same_vertices(rp.read_model_vertices(), a)
    rp.update_model_vertices(pts, nrm)                             # unposed again: as before this feature
    assert _same_vertices(rp.read_model_vertices(), dict(points=pts, normals=nrm))
    rp.set_model_pose(m)                                           # and the next pose starts from what the slot then held
    assert _same_vertices(rp.read_model_vertices(), _posed(dict(a, points=pts, normals=nrm), m))
    rp.close()


# ---- 5. device source ------------------------------------------------------------------------------
class Hip:
    """the few HIP calls this file needs to put vertex data into device memory behind a stream of its own"""
    H2D, D2H = 1, 2

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        assert self.hip.hipSetDevice(0) == 0
        self.stream = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(self.stream)) == 0
        self.allocs, self.pinned = [], []

    def upload(self, array, stream=True):
        """device pointer (int) of a copy of `array`: an async copy from pinned memory on self.stream, or a synchronous one"""
        a = np.ascontiguousarray(array)
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), C.c_size_t(max(a.nbytes, 16))) == 0
        self.allocs.append(d)
        if stream:
            h = C.c_void_p()
            assert self.hip.hipHostMalloc(C.byref(h), C.c_size_t(max(a.nbytes, 16)), 0) == 0
            self.pinned.append(h)
            C.memmove(h, a.ctypes.data, a.nbytes)
            assert self.hip.hipMemcpyAsync(d, h, C.c_size_t(a.nbytes), self.H2D, self.stream) == 0
        else:
            assert self.hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), self.H2D) == 0
        return d.value

    def close(self):
        assert self.hip.hipSetDevice(0) == 0
        assert self.hip.hipStreamSynchronize(self.stream) == 0
        for d in self.allocs:
            self.hip.hipFree(d)
        for h in self.pinned:
            self.hip.hipHostFree(h)
        self.hip.hipStreamDestroy(self.stream)


def test_vertex_update_from_device_memory(mesh_dir):
    tex, cfg = T.textures(), _small()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    pts, nrm = _other_geometry(a)
    np_, nn = len(pts), len(nrm)
    hip = Hip()
    for m in (None, _pose(1)):                                     # an unposed slot and a posed one
        host = _ctx(cfg, tex)
        host.upload_model_build(a); host.set_uniforms(*u)
        if m is not None:
            host.set_model_pose(m)
        host.update_model_vertices(pts, nrm)
        want = _state(host)
        host.update_model_vertices(points=a["points"])
        want_one = _state(host)
        host.close()
        if m is not None:
            assert _same_vertices(want[0], _posed(dict(points=pts, normals=nrm), m))
        rp = _ctx(cfg, tex)
        rp.upload_model_build(a); rp.set_uniforms(*u)
        if m is not None:
            rp.set_model_pose(m)
        rp.update_model_vertices_device(hip.upload(pts), hip.upload(nrm), np_, nn, stream=hip.stream.value)
        got = _state(rp)
        assert _same_vertices(got[0], want[0]) and _same_tree(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2])), m is not None
        rp.update_model_vertices_device(hip.upload(a["points"]), None, np_, 0, stream=hip.stream.value)      # None keeps the normals
        got = _state(rp)
        assert _same_vertices(got[0], want_one[0]) and _same_tree(got[1], want_one[1]) and np.array_equal(_bits(got[2]), _bits(want_one[2])), m is not None
        rp.update_model_vertices_device(hip.upload(pts, stream=False), hip.upload(nrm, stream=False), np_, nn)     # the legacy stream, after a synchronous copy
        got = _state(rp)
        assert _same_vertices(got[0], want[0]) and _same_tree(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2])), m is not None
        rp.close()
    rp = _ctx(cfg, tex)
    rp.upload_model_build(a); rp.set_uniforms(*u)
    before = _state(rp)
    dp, dn = hip.upload(pts, stream=False), hip.upload(nrm, stream=False)
    assert _code(lambda: rp.update_model_vertices_device(dp, dn, np_ - 1, nn)) == E_INVALID
    assert _code(lambda: rp.update_model_vertices_device(dp, dn, np_, nn + 1)) == E_INVALID
    assert _code(lambda: rp.update_model_vertices_device(dp, dn, np_, nn, index=8)) == E_INVALID
    assert _code(lambda: rp.update_model_vertices_device(dp, dn, np_, nn, index=5)) == E_STATE            # empty slot
    rp.upload_model(B.load_model(str(mesh_dir / "sphere_24_32.obj")), 1)
    assert _code(lambda: rp.update_model_vertices_device(dp, dn, np_, nn, index=1)) == E_STATE            # host-built slot
    after = _state(rp)
    assert _same_vertices(after[0], before[0]) and _same_tree(after[1], before[1]) and np.array_equal(_bits(after[2]), _bits(before[2]))
    rp.close()
    hip.close()


# ---- 6. every frame mode ---------------------------------------------------------------------------
def _animation(a, cfg, tex, bind=True, **kw):
    rp = _ctx(cfg, tex, **kw)
    rp.upload_model_build(a)
    w, h = cfg.frame_w, cfg.frame_h
    bufs, out = [], []
    for k in range(4):                                             # pose 0 = never posed; with bound outputs nothing is read in between
        if k > 0:
            rp.set_model_pose(_pose(k))
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


def test_frame_k_shows_pose_k_in_every_frame_mode(mesh_dir):
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


# ---- 7. partitions ---------------------------------------------------------------------------------
def test_partitioned_ctx_gathers_the_single_ctx_posed_frame(mesh_dir):
    tex = T.textures()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    cfg = B.ladder_for_frame((320, 180), 3, 3)
    m = _pose(1)
    one = _ctx(cfg, tex, frames_in_flight=1)
    one.upload_model_build(a); one.set_uniforms(*u)
    one.render()
    plain = one.read_hdr().copy()
    one.set_model_pose(m)
    verts, tree, want = _state(one)
    one.close()
    assert not np.array_equal(_bits(plain), _bits(want))
    modes = [dict(devices=[0] * 8, stripe_rows=9, frames_per_batch=2, frames_in_flight=2)]
    if B.lib().bhray_device_count() >= 2:
        modes.append(dict(devices=[0, 1], stripe_rows=9, frames_in_flight=2))
    for kw in modes:
        rp = _ctx(cfg, tex, **kw)
        rp.upload_model_build(a); rp.set_uniforms(*u)
        for _ in range(3):
            rp.render()
        rp.set_model_pose(m)
        rp.render()
        assert np.array_equal(_bits(rp.read_hdr()), _bits(want)), kw
        assert _same_vertices(rp.read_model_vertices(), verts) and _same_tree(rp.read_model_bvh(), tree), kw
        rp.set_model_pose(None)
        rp.render()
        assert np.array_equal(_bits(rp.read_hdr()), _bits(plain)), kw
        rp.close()


# ---- 8. lensed -------------------------------------------------------------------------------------
def test_posed_slot_under_mesh_lensing(mesh_dir):
    tex = T.textures()
    p = os.path.join(str(mesh_dir), "ico1_8.obj")
    with open(p, "w") as f:
        f.write(assets.icosphere_mesh_obj(1, radius=8.0))          # 80 triangles
    model = B.load_model(p)
    model.set_transform((-10.0, 0.0, 17.0), 1)                     # straddles the relativity sphere (R = 20) in front of the default camera
    a = {k: model.arrays()[k] for k in ("position", "visible", "points", "normals", "triangles")}
    cfg = B.ladder_from_base((32, 18), 3, 1)
    m = PR.from_euler((0.5, -0.4, 0.3), (1.0, 0.0, -1.0), 1.1)
    for method in (1, 0):
        u = T.uniforms(integration_method=method, model_count=1)
        frames = []
        for posed_on_device in (True, False):
            rp = _ctx(cfg, tex)
            rp.set_mesh_lensing(True)
            rp.set_uniforms(*u)
            if posed_on_device:
                rp.upload_model_build(a)
                rp.render()
                frames.append(rp.read_hdr().copy())
                rp.set_model_pose(m)
            else:
                rp.upload_model_build(_posed(a, m))
            rp.render()
            frames.append(rp.read_hdr().copy())
            rp.close()
        rest, posed, fresh = frames
        assert np.array_equal(_bits(posed), _bits(fresh)), method
        assert not np.array_equal(_bits(rest), _bits(posed)), method
        flat = _ctx(cfg, tex)
        flat.set_uniforms(*u)
        flat.upload_model_build(_posed(a, m))
        flat.render()
        assert not np.array_equal(_bits(flat.read_hdr()), _bits(posed)), method       # the lensed steps see the posed mesh
        flat.close()


# ---- 9. errors keep the slot -----------------------------------------------------------------------
def test_errors_are_codes_and_keep_the_slot(mesh_dir):
    tex, cfg = T.textures(), _small()
    a = R.case_arrays("sphere_24_32", mesh_dir)
    u = T.uniforms(camera=_camera(), integration_method=1, model_count=1)
    rp = _ctx(cfg, tex)
    rp.upload_model_build(a); rp.set_uniforms(*u)
    rp.set_model_pose(_pose(1))
    before = _state(rp)
    for i, bad in ((0, np.nan), (7, np.inf), (11, -np.inf), (3, np.nan)):
        m = _pose(2).copy()
        m.reshape(-1)[i] = bad
        assert _code(lambda: rp.set_model_pose(m)) == E_INVALID, (i, bad)
    assert _code(lambda: rp.set_model_pose(_pose(2), index=8)) == E_INVALID
    assert _code(lambda: rp.set_model_pose(None, index=8)) == E_INVALID
    assert _code(lambda: rp.set_model_pose(_pose(2), index=5)) == E_STATE                 # empty slot
    assert _code(lambda: rp.set_model_pose(None, index=5)) == E_STATE
    rp.upload_model(B.load_model(str(mesh_dir / "sphere_24_32.obj")), 1)
    assert _code(lambda: rp.set_model_pose(_pose(2), index=1)) == E_STATE                 # host-built slot
    assert _code(lambda: rp.read_model_vertices(5)) == E_STATE and _code(lambda: rp.read_model_vertices(8)) == E_INVALID
    after = _state(rp)
    assert _same_vertices(after[0], before[0]) and _same_tree(after[1], before[1]) and np.array_equal(_bits(after[2]), _bits(before[2]))
    host = rp.read_model_vertices(1)                               # any slot can be read: a host-built one holds what was uploaded
    assert _same_vertices(host, B.load_model(str(mesh_dir / "sphere_24_32.obj")).arrays())
    npts, nnrm = C.c_uint32(), C.c_uint32()
    small = np.zeros((4, 4), dtype=np.float32)
    L, h = rp._L, rp._h
    assert L.bhray_read_model_vertices(h, 0, small.ctypes.data, 4, None, 0, C.byref(npts), C.byref(nnrm)) == E_INVALID
    assert (npts.value, nnrm.value) == (len(a["points"]), len(a["normals"]))               # caps too small: the counts are still written
    npts.value = nnrm.value = 0
    assert L.bhray_read_model_vertices(h, 0, None, 0, small.ctypes.data, 4, C.byref(npts), C.byref(nnrm)) == E_INVALID
    assert (npts.value, nnrm.value) == (len(a["points"]), len(a["normals"]))
    assert not small.any()
    only_n = np.zeros((len(a["normals"]), 4), dtype=np.float32)    # either pointer may be NULL: that array is not read
    assert L.bhray_read_model_vertices(h, 0, None, 0, only_n.ctypes.data, len(only_n), None, None) == 0
    assert np.array_equal(_bits(only_n), _bits(before[0]["normals"]))
    rp.upload_model_build(dict(a, triangles=a["triangles"][:0]), 2)                        # 0 triangles: no arrays, nothing to pose
    assert _code(lambda: rp.set_model_pose(_pose(1), index=2)) == E_STATE
    empty = rp.read_model_vertices(2)
    assert empty["points"].shape == (0, 4) and empty["normals"].shape == (0, 4)
    rp.close()


# ---- 10. hosts -------------------------------------------------------------------------------------
def test_renderer_set_model_rotation_and_save_image(mesh_dir, tmp_path):
    from PIL import Image
    tex = T.textures()
    R.case_arrays("sphere_24_32", mesh_dir)
    model = B.load_model(str(mesh_dir / "sphere_24_32.obj"))
    cfg = B.ladder_from_base((24, 14), 3, 3)                       # 208 x 118: no crop, wide enough for the bloom chain
    rotation, pivot, scale = (0.3, 0.7, -0.2), (0.5, 0.0, -0.5), 1.2
    r = B.Renderer(cfg, device=0)
    r.ray_pass.set_textures(*tex)
    r.camera = _camera()
    r.ray_details.integration_method = 1
    assert r.add_model(model, build="device") == 0
    r.render()
    rest = r.read_hdr().copy()
    r.set_model_rotation(0, rotation, pivot, scale)
    r.render()
    got = r.read_hdr().copy()
    a = {k: model.arrays()[k] for k in ("position", "visible", "points", "normals", "triangles")}
    want_arrays = _posed(a, B.pose_from_euler(rotation, pivot, scale))
    assert _same_vertices(r.ray_pass.read_model_vertices(0), want_arrays)
    fresh = _ctx(cfg, tex)
    fresh.upload_model_build(want_arrays)
    fresh.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    fresh.render()
    assert np.array_equal(_bits(got), _bits(fresh.read_hdr())) and not np.array_equal(_bits(got), _bits(rest))
    fresh.close()
    png = tmp_path / "posed.png"
    r.save_image(str(png))
    sky = r.ray_pass.read_sky()
    f, m = B.post_defaults()
    want = PO.post_ref(sky, (np.float32(f.edge_threshold_min), np.float32(f.edge_threshold_max), int(f.iterations), np.float32(f.subpixel_quality)), np.float32(m.mix_ratio))
    want[..., 3] = 255
    assert np.array_equal(np.asarray(Image.open(png).convert("RGBA")), want)
    host = B.Renderer(cfg, device=0)
    assert host.add_model(model) == 0 and host.add_model(model, build="device") == 1
    with pytest.raises(ValueError):
        host.set_model_rotation(0, rotation)                       # built on the host
    with pytest.raises(ValueError):
        host.set_model_rotation(2, rotation)
    host.set_model_rotation(1, rotation)
    host.set_model(model)
    with pytest.raises(ValueError):
        host.set_model_rotation(0, rotation)
    r.ray_pass.close(); host.ray_pass.close()


def test_cpp_host_program_with_pose(mesh_dir, tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    R.case_arrays("sphere_24_32", mesh_dir)
    obj = str(mesh_dir / "sphere_24_32.obj")
    base = [exe, str(tmp_path / "posed.f32"), "--rk", "--base", "24", "14", "--levels", "3", "--disk-size", "64", "--obj", obj]
    r = subprocess.run(base + ["--bvh", "device", "--pose", "0.3", "0.7", "-0.2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w, h = (int(v) for v in r.stdout.strip().splitlines()[-1].split("x"))
    got = np.fromfile(tmp_path / "posed.f32", dtype=np.float32).reshape(h, w, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)      # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((24, 14), 3, 3), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.add_model(B.load_model(obj), build="device")
    r2.ray_details.integration_method = 1
    r2.render()
    rest = r2.read_hdr().copy()
    r2.set_model_rotation(0, (0.3, 0.7, -0.2))
    r2.render()
    assert np.array_equal(_bits(got), _bits(r2.read_hdr())) and not np.array_equal(_bits(got), _bits(rest))
    r2.ray_pass.close()
    for args in (["--pose", "0.3", "0.7", "-0.2"], ["--bvh", "reference", "--pose", "0.3", "0.7", "-0.2"]):      # --pose needs --bvh device
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--bvh device" in bad.stderr, args


# ---- 11. build info --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico4", "bench"])
def test_build_info_after_a_pose(mesh_dir, name):
    a = R.case_arrays(name, mesh_dir)
    m = _pose(1)
    rp = _ctx(B.ladder_from_base((24, 14), 3, 2), T.textures())
    rp.upload_model_build(a)
    rp.set_model_pose(m)
    info = rp.model_build_info()
    print(f"{name} posed: {info}")
    if name == "ico4":
        want = R.build(_posed(a, m)["points"], a["triangles"])
        counts = (len(want["nodes"]), want["leaves"], want["max_leaf"], want["max_depth"])
    else:                                                          # the restatement takes seconds at this size: the counts of a fresh build of the same arrays
        rp.upload_model_build(_posed(a, m), 1)
        f = rp.model_build_info(1)
        counts = (f["nodes"], f["leaves"], f["max_leaf"], f["max_depth"])
    assert (info["built_on_device"], info["triangles"]) == (1, len(a["triangles"]))
    assert (info["nodes"], info["leaves"], info["max_leaf"], info["max_depth"]) == counts
    assert info["build_ms"] > 0.0 and info["upload_ms"] >= 0.0
    rp.close()
