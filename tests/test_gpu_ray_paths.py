"""-m gpu: ray paths (bhray_trace_rays_paths, bhray_trace_rays_paths_device).

  1. Every point to the bit: 1 027 rays of arbitrary origin at stride 1 against the NumPy restatement (tests/ray_paths_ref.py) - counts, every iteration word, every
     position word; results and records are bhray_trace_rays_records' for the same rays.
  2. Strides 2^3 and 2^16 are the stride-1 run's points with iteration % 2^s == 0 and its end point.
  3. A row that is too short is cut, the counts are not, and no byte outside a ray's own points is written (a 0xA5 pattern and guard regions round the device arrays).
  4. Meshes (two visible slots, one invisible), RK.       5. n = 0, 1, 63, 64, 65.       6. The device form on a stream of the caller's; unusable rays.
  7. Frames around a paths batch keep their bits; a model upload waits for an outstanding batch.       8. The refused states and arguments.
  9. Renderer.ray_path and the C++ host's --path."""
import ctypes as C
import functools

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T
from tests import ray_paths_ref as PR
from tests import ray_records_ref as R
from tests import rays_ref as RR
from tests.test_gpu_trace_rays import _Hip, _with_unusable_rays

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
N = PR.N_SEEDED
MAXP = PR.MAX_POINTS
PATTERN = 0xA5
PATTERN_WORD = 0xA5A5A5A5
GUARD = 4096


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rec_words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)


def _pt_words(points):
    """(n, max_points, 4) uint32 over an (n, max_points) PATH_POINT_DTYPE array"""
    p = np.ascontiguousarray(points)
    return p.view(np.uint32).reshape(p.shape[0], -1, 4)


def _ctx(cfg=None, **kw):
    rp = B.RayPass(cfg if cfg is not None else B.ladder_from_base((24, 14), 3, 1), **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*T.textures())
    return rp


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _rays():
    return RR.seeded_rays()[:N]


@functools.lru_cache(maxsize=None)
def _gpu_seeded(method, s=0):
    """the host form over the seeded list at stride 2^s, MAXP points per row: (ctx, results, records, points, counts), computed once"""
    rp = _ctx()
    rp.set_uniforms(*RR.scene_uniforms(method))
    got = rp.trace_rays_paths(_rays(), s, MAXP)
    for a in got:
        a.setflags(write=False)
    return (rp,) + got


def _keep(margin):
    keep = margin >= R.MARGIN_BAR
    assert int((~keep).sum()) <= R.MARGIN_SHARE * margin.shape[0], "too many rays whose break test sits on its threshold"
    return keep


def _assert_points(points, counts, paths, s, keep, what):
    """the whole rows - points, and the zero slots behind them - and the counts against the restatement, word for word, on the rays kept"""
    want, want_counts = PR.rows(paths, s, points.shape[1])
    bad_counts = int((counts != want_counts)[keep].sum())
    g, w = _pt_words(points), _pt_words(want)
    bad_iter = int((g[..., 3] != w[..., 3]).any(axis=1)[keep].sum())
    bad_pos = int((g[..., 0:3] != w[..., 0:3]).any(axis=(1, 2))[keep].sum())
    print(f"{what}: of {int(keep.sum())} rays compared ({int((~keep).sum())} left out) the counts differ on {bad_counts}, an iteration word on {bad_iter}, "
          f"a position word on {bad_pos}; {int(want_counts[keep].sum())} points, the longest row {int(want_counts.max())}")
    assert bad_counts == 0, f"{what}: counts differ from the restatement on {bad_counts} rays"
    assert bad_iter == 0, f"{what}: iteration words differ from the restatement on {bad_iter} rays"
    assert bad_pos == 0, f"{what}: position words differ from the restatement on {bad_pos} rays"


# ---- 1. every point to the bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_every_point_matches_the_restatement(method):
    _, want_rec, margin, _, paths, want_counts = PR.seeded_reference(method)
    assert int(want_counts.max()) <= MAXP, "nothing may be dropped at stride 1"
    keep = _keep(margin)
    rp, out, rec, points, counts = _gpu_seeded(method)
    assert points.shape == (N, MAXP) and points.dtype == B.PATH_POINT_DTYPE and counts.shape == (N,) and counts.dtype == np.uint32
    _assert_points(points, counts, paths, 0, keep, f"method {method}")
    assert np.array_equal(counts, rec["iterations"] + 2), "counts[r] = (iterations >> 0) + 2"
    plain_out, plain_rec = rp.trace_rays_records(_rays())
    assert np.array_equal(_bits(out), _bits(plain_out)), "the results are not bhray_trace_rays_records' for the same rays"
    assert np.array_equal(_rec_words(rec), _rec_words(plain_rec)), "the records are not bhray_trace_rays_records' for the same rays"
    # the end point: the record's iterations, and for a ray that hit nothing the record's position
    last = points[np.arange(N), counts - 1]
    assert np.array_equal(last["iteration"], rec["iterations"])
    none = (rec["hit"] & 0xFF) == B.HIT_NONE
    assert none.sum() >= 100 and np.array_equal(_bits(last["position"][none]), _bits(rec["position"][none]))


# ---- 2. strides -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [3, 16])
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_a_stride_keeps_every_2_to_the_s_th_point_and_the_end(method, s):
    _, _, margin, _, paths, _ = PR.seeded_reference(method)
    _, out1, rec1, points1, counts1 = _gpu_seeded(method)
    _, out, rec, points, counts = _gpu_seeded(method, s)
    assert np.array_equal(_bits(out), _bits(out1)) and np.array_equal(_rec_words(rec), _rec_words(rec1))
    # GPU against GPU, every ray: the stride-1 run's own points, sampled
    own = [points1[r, :counts1[r]] for r in range(N)]
    want, want_counts = PR.rows(own, s, MAXP)
    assert np.array_equal(counts, want_counts) and np.array_equal(counts, (rec["iterations"] >> s) + 2)
    assert np.array_equal(_pt_words(points), _pt_words(want)), "the strided points are not the stride-1 run's"
    _assert_points(points, counts, paths, s, _keep(margin), f"method {method}, stride 2^{s}")
    if s == 16:
        assert (counts == 2).all(), "a stride beyond every ray's length leaves the origin and the end point"
        assert (points["iteration"][:, 0] == 0).all() and np.array_equal(points["iteration"][:, 1], rec["iterations"])


# ---- the device form ----------------------------------------------------------------------------------------
def _device_paths(rp, hip, rays, s, max_points, stream=True):
    """the device form over `rays` with the point and count arrays inside guard regions, everything pre-filled with the pattern:
    (results, records, points, counts, guards_intact)"""
    n = rays.shape[0]
    src = np.ascontiguousarray(rays)
    pbytes, cbytes = n * max_points * 16, n * 4
    d_rays, d_out, d_rec = hip.alloc(n * 32), hip.alloc(n * 16), hip.alloc(n * 32)
    d_pts, d_cnt = hip.alloc(pbytes + 2 * GUARD), hip.alloc(cbytes + 2 * GUARD)
    st = hip.stream
    assert hip.hip.hipMemcpyAsync(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D, st) == 0
    assert hip.hip.hipMemsetAsync(d_pts, PATTERN, C.c_size_t(pbytes + 2 * GUARD), st) == 0
    assert hip.hip.hipMemsetAsync(d_cnt, PATTERN, C.c_size_t(cbytes + 2 * GUARD), st) == 0
    if not stream:                                                # the legacy stream: the fills above are on a non-blocking stream, which it does not wait for
        assert hip.hip.hipStreamSynchronize(st) == 0
    rp.trace_rays_paths_device(d_rays.value, n, s, max_points, d_out.value, d_rec.value, d_pts.value + GUARD, d_cnt.value + GUARD, stream=st.value if stream else None)
    if not stream:
        rp.sync()                                                 # ... nor do the copies below wait for it: bhray_sync waits for an outstanding batch
    out = np.zeros((n, 4), dtype=np.float32)
    rec = np.zeros(n, dtype=B.RAY_RECORD_DTYPE)
    pts = np.zeros(pbytes // 4 + 2 * GUARD // 4, dtype=np.uint32)
    cnt = np.zeros(n + 2 * GUARD // 4, dtype=np.uint32)
    for host, dev in ((out, d_out), (rec, d_rec), (pts, d_pts), (cnt, d_cnt)):
        assert hip.hip.hipMemcpyAsync(C.c_void_p(host.ctypes.data), dev, C.c_size_t(host.nbytes), hip.D2H, st) == 0
    assert hip.hip.hipStreamSynchronize(st) == 0
    rp.sync()
    g = GUARD // 4
    intact = bool((pts[:g] == PATTERN_WORD).all() and (pts[-g:] == PATTERN_WORD).all() and (cnt[:g] == PATTERN_WORD).all() and (cnt[-g:] == PATTERN_WORD).all())
    points = pts[g:-g].view(B.PATH_POINT_DTYPE).reshape(n, max_points)
    return out, rec, points, cnt[g:-g].copy(), intact


def _assert_rows_cut(points, counts, full_points, full_counts, max_points, rows):
    """rows: the first min(count, max_points) points are the full run's, every other word of the row still holds the pattern"""
    w, fw = _pt_words(points), _pt_words(full_points)
    for r in rows:
        k = min(int(full_counts[r]), max_points)
        assert int(counts[r]) == int(full_counts[r]), (r, counts[r], full_counts[r])
        assert np.array_equal(w[r, :k], fw[r, :k]), f"ray {r}: the first {k} points differ"
        assert (w[r, k:] == PATTERN_WORD).all(), f"ray {r}: a slot behind point {k - 1} was written"


# ---- 3. truncation, and no store outside a row -----------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_a_short_row_is_cut_and_nothing_else_is_written(method):
    rp, out1, rec1, points1, counts1 = _gpu_seeded(method)
    assert int((counts1 > 5).sum()) >= N // 2, "most rows must be cut"
    hip = _Hip()
    try:
        out, rec, points, counts, intact = _device_paths(rp, hip, _rays(), 0, 5)
        assert intact, "a guard region was written"
        assert np.array_equal(counts, counts1), "the counts do not depend on max_points"
        _assert_rows_cut(points, counts, points1, counts1, 5, range(N))
        assert np.array_equal(_bits(out), _bits(out1)) and np.array_equal(_rec_words(rec), _rec_words(rec1))
    finally:
        hip.close()


# ---- 4. meshes --------------------------------------------------------------------------------------------
def test_meshes():
    _, want_rec, margin, after_march, paths, want_counts = PR.mesh_reference(1)
    assert int(want_counts.max()) <= MAXP
    keep = _keep(margin)
    c = R.mesh_conditions(want_rec, after_march)
    assert c["mesh_slot0"] >= 150 and c["mesh_slot2"] >= 150 and c["after_march"] >= 50 and c["mesh_slot1"] == 0, c
    rp = _ctx()
    for slot, m in enumerate(R.mesh_models()):
        rp.upload_model(m, slot)
    rp.set_uniforms(*R.mesh_uniforms(1))
    out, rec, points, counts = rp.trace_rays_paths(R.mesh_rays(), 0, MAXP)
    _assert_points(points, counts, paths, 0, keep, "meshes, rk")
    plain_out, plain_rec = rp.trace_rays_records(R.mesh_rays())
    assert np.array_equal(_bits(out), _bits(plain_out)) and np.array_equal(_rec_words(rec), _rec_words(plain_rec))
    mesh = (rec["hit"] & 0xFF) == B.HIT_MESH
    last = points[np.arange(rec.shape[0]), counts - 1]
    assert mesh.sum() >= 300 and np.array_equal(_bits(last["position"][mesh]), _bits(rec["position"][mesh])), "a mesh hit ends the ray where the record says"


# ---- 5. sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_a_rays_path_does_not_depend_on_its_batch(method):
    rp, out1, rec1, points1, counts1 = _gpu_seeded(method)
    for n in (1, 63, 64, 65):
        out, rec, points, counts = rp.trace_rays_paths(_rays()[:n], 0, MAXP)
        assert points.shape == (n, MAXP) and counts.shape == (n,)
        assert np.array_equal(counts, counts1[:n]) and np.array_equal(_pt_words(points), _pt_words(points1[:n])), f"n = {n}: the paths differ from the prefix of the full batch"
        assert np.array_equal(_rec_words(rec), _rec_words(rec1[:n])) and np.array_equal(_bits(out), _bits(out1[:n]))
    out, rec, points, counts = rp.trace_rays_paths(_rays()[:0], 0, MAXP)
    assert out.shape == (0, 4) and rec.shape == (0,) and points.shape == (0, MAXP) and counts.shape == (0,)
    # n == 0 with arrays given: nothing is touched
    src = np.ascontiguousarray(_rays()[:4])
    o = np.full((4, 4), 7.0, np.float32); r = np.zeros(4, B.RAY_RECORD_DTYPE); r["iterations"] = 77
    p = np.full(4 * 8 * 4, PATTERN_WORD, np.uint32); c = np.full(4, PATTERN_WORD, np.uint32)
    rc = B.lib().bhray_trace_rays_paths(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), 0, 0, 8, o.ctypes.data_as(C.POINTER(C.c_float)),
                                        r.ctypes.data_as(C.POINTER(B.BhrayRayRecord)), p.ctypes.data_as(C.POINTER(B.BhrayPathPoint)), c.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0 and (o == 7.0).all() and (r["iterations"] == 77).all() and (p == PATTERN_WORD).all() and (c == PATTERN_WORD).all()
    # the results and the records may be left out (NULL)
    p = np.zeros((65, MAXP), B.PATH_POINT_DTYPE); c = np.zeros(65, np.uint32)
    src = np.ascontiguousarray(_rays()[:65])
    rc = B.lib().bhray_trace_rays_paths(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), 65, 0, MAXP, None, None, p.ctypes.data_as(C.POINTER(B.BhrayPathPoint)),
                                        c.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0 and np.array_equal(c, counts1[:65]) and np.array_equal(_pt_words(p), _pt_words(points1[:65]))


# ---- 6. the device form on a caller's stream, unusable rays -----------------------------------------------
def test_device_form_on_a_callers_stream_and_unusable_rays():
    rp, out1, rec1, points1, counts1 = _gpu_seeded(1)
    special, bad = _with_unusable_rays(_rays())
    unusable = [bad["nan_origin"], bad["inf_direction"], bad["zero_direction"]]
    assert max(bad.values()) < N
    hip = _Hip()
    try:
        out, rec, points, counts, intact = _device_paths(rp, hip, special, 0, MAXP)
        assert intact, "a guard region was written"
        for k in unusable:
            assert out[k].tolist() == [0.0, 0.0, 0.0, -1.0], (k, out[k])
            assert _rec_words(rec[k:k + 1])[0].tolist() == [0, 0, 0, B.HIT_UNUSABLE, 0xFFFFFFFF, 0, 0, 0], (k, rec[k])
            assert int(counts[k]) == 0, (k, counts[k])
            assert (_pt_words(points)[k] == PATTERN_WORD).all(), f"unusable ray {k}: a point was written"
        usable = [r for r in range(N) if r not in unusable]
        _assert_rows_cut(points, counts, points1, counts1, MAXP, usable)
        assert np.array_equal(_rec_words(rec[usable]), _rec_words(rec1[usable])) and np.array_equal(_bits(out[usable]), _bits(out1[usable]))
        assert int(counts[bad["nan_pad"]]) == int(counts1[bad["nan_pad"]]) >= 2, "the pad words are not looked at"
        # the host form refuses the same list as a whole and leaves its outputs alone
        src = np.ascontiguousarray(special)
        p = np.full(N * 2 * 4, PATTERN_WORD, np.uint32); c = np.full(N, PATTERN_WORD, np.uint32)
        rc = B.lib().bhray_trace_rays_paths(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), N, 0, 2, None, None, p.ctypes.data_as(C.POINTER(B.BhrayPathPoint)),
                                            c.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == E_INVALID and (p == PATTERN_WORD).all() and (c == PATTERN_WORD).all()
        # the legacy stream (no stream given) serves as well
        out, rec, points, counts, intact = _device_paths(rp, hip, _rays()[:65], 3, 16, stream=False)
        assert intact and np.array_equal(counts, (rec1["iterations"][:65] >> 3) + 2)
    finally:
        hip.close()


# ---- 7. state ---------------------------------------------------------------------------------------------
def test_frames_before_and_after_a_paths_batch_keep_their_bits():
    cfg = B.ladder_from_base((40, 24), 3, 2)
    cams = [B.Camera(position=(0.0, 0.0, -19.0)), B.Camera(position=(1.0, 0.5, -30.0), forward=(0.0, 0.05, 1.0))]

    def run(with_batch):
        rp = _ctx(cfg, frames_in_flight=4)
        first = B.PinnedFrame(len(rp.local_rows()), rp.frame_size[0])
        rp.set_uniforms(*T.uniforms(camera=cams[0], integration_method=1))
        rp.render()
        ticket = rp.read_hdr_async(first)
        batch = rp.trace_rays_paths(_rays()[:500], 0, MAXP) if with_batch else None
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
        assert np.array_equal(_bits(plain[k]), _bits(mixed[k])), f"frame {k} changed with a paths batch between the renders"
    # (the batch ran under the first frame's uniforms, the seeded reference under rays_ref.scene_uniforms: the same hole, the same details)
    _, out1, rec1, points1, counts1 = _gpu_seeded(1)
    assert np.array_equal(batch[3], counts1[:500]) and np.array_equal(_pt_words(batch[2]), _pt_words(points1[:500])), "the batch between two frames differs from the batch alone"
    assert np.array_equal(_rec_words(batch[1]), _rec_words(rec1[:500]))


def test_a_model_upload_waits_for_an_outstanding_paths_batch():
    rays = R.mesh_rays()
    n = rays.shape[0]
    old, new = RR.mesh_model(R.MESH_SLOTS[0]), RR.mesh_model((0.0, -90.0, 5.0))
    rp = _ctx()
    rp.upload_model(old)
    rp.set_uniforms(*RR.scene_uniforms(1, 1))
    want = rp.trace_rays_paths(rays, 0, MAXP)
    hip = _Hip()
    try:
        d_rays, d_out, d_rec, d_pts, d_cnt = hip.alloc(n * 32), hip.alloc(n * 16), hip.alloc(n * 32), hip.alloc(n * MAXP * 16), hip.alloc(n * 4)
        src = np.ascontiguousarray(rays)
        assert hip.hip.hipMemcpy(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D) == 0
        assert hip.hip.hipMemsetAsync(d_pts, 0, C.c_size_t(n * MAXP * 16), hip.stream) == 0
        rp.trace_rays_paths_device(d_rays.value, n, 0, MAXP, d_out.value, d_rec.value, d_pts.value, d_cnt.value, stream=hip.stream.value)
        rp.upload_model(new)                                      # with the batch outstanding: must wait for it, not pull the old model from under it
        pts = np.zeros((n, MAXP), B.PATH_POINT_DTYPE); cnt = np.zeros(n, np.uint32); rec = np.zeros(n, B.RAY_RECORD_DTYPE)
        for host, dev in ((pts, d_pts), (cnt, d_cnt), (rec, d_rec)):
            assert hip.hip.hipMemcpyAsync(C.c_void_p(host.ctypes.data), dev, C.c_size_t(host.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipStreamSynchronize(hip.stream) == 0
        assert np.array_equal(cnt, want[3]) and np.array_equal(_pt_words(pts), _pt_words(want[2])), "the outstanding batch did not see the OLD model"
        assert np.array_equal(_rec_words(rec), _rec_words(want[1]))
        after = rp.trace_rays_paths(rays, 0, MAXP)
        assert int((_pt_words(after[2]) != _pt_words(want[2])).any(axis=(1, 2)).sum()) >= 100, "the two models must differ in the rays' paths"
        rp.sync()
    finally:
        hip.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------
def test_refused_states_are_those_of_trace_rays():
    rays = _rays()[:65]
    u = RR.scene_uniforms(1)
    rp = _ctx()
    assert _code(lambda: rp.trace_rays_paths(rays, 0, 16)) == E_STATE           # before the first set_uniforms
    rp.set_uniforms(*u)
    good = rp.trace_rays_paths(rays, 0, MAXP)
    for kw in ({"literal": True}, {"eval_fma": True}):
        q = _ctx(**kw)
        q.set_uniforms(*u)
        assert _code(lambda: q.trace_rays_paths(rays, 0, 16)) == E_STATE, kw
    rp.set_mesh_lensing(True)
    assert _code(lambda: rp.trace_rays_paths(rays, 0, 16)) == E_STATE
    rp.set_mesh_lensing(False)
    again = rp.trace_rays_paths(rays, 0, MAXP)
    assert np.array_equal(_pt_words(again[2]), _pt_words(good[2])) and np.array_equal(again[3], good[3])
    multi = _ctx(devices=[0, 0])
    multi.set_uniforms(*u)
    assert _code(lambda: multi.trace_rays_paths(rays, 0, 16)) == E_STATE
    assert _code(lambda: rp.trace_rays_paths(np.full((1, 6), np.nan, np.float32), 0, 16)) == E_INVALID
    counting = _ctx(counters=True)                                         # the kernels that do not count: its counters do not move
    counting.set_uniforms(*u)
    counting.render(); counting.sync()
    before = counting.counters()
    got = counting.trace_rays_paths(rays, 0, MAXP)
    assert np.array_equal(_pt_words(got[2]), _pt_words(good[2])) and np.array_equal(got[3], good[3])
    assert counting.counters() == before


def test_refused_arguments_leave_the_outputs_alone():
    L = B.lib()
    rp = _ctx()
    rp.set_uniforms(*RR.scene_uniforms(1))
    big = np.zeros((65536, 8), np.float32); big[:, 6] = 1.0; big[:65] = _rays()[:65]
    o = np.full((65, 4), 7.0, np.float32); r = np.zeros(65, B.RAY_RECORD_DTYPE); r["iterations"] = 77
    p = np.full(65 * 16 * 4, PATTERN_WORD, np.uint32); c = np.full(65, PATTERN_WORD, np.uint32)
    ptr = dict(rays=big.ctypes.data_as(C.POINTER(B.BhrayRay)), out=o.ctypes.data_as(C.POINTER(C.c_float)), rec=r.ctypes.data_as(C.POINTER(B.BhrayRayRecord)),
               pts=p.ctypes.data_as(C.POINTER(B.BhrayPathPoint)), cnt=c.ctypes.data_as(C.POINTER(C.c_uint32)))

    def host(n=65, s=0, mp=16, **kw):
        a = dict(ptr, **kw)
        return L.bhray_trace_rays_paths(rp._h, a["rays"], n, s, mp, a["out"], a["rec"], a["pts"], a["cnt"])

    cases = {"max_points 0": host(mp=0), "max_points 1": host(mp=1), "stride_log2 17": host(s=17), "n * max_points over the limit": host(n=4097, mp=4096),
             "n * max_points = 2^32": host(n=65536, mp=65536), "n over its limit": host(n=(1 << 26) + 1, mp=2), "NULL points": host(pts=None), "NULL counts": host(cnt=None),
             "NULL rays": host(rays=None)}
    assert all(rc == E_INVALID for rc in cases.values()), cases
    assert (o == 7.0).all() and (r["iterations"] == 77).all() and (p == PATTERN_WORD).all() and (c == PATTERN_WORD).all(), "a refused call touched an output"
    assert host() == 0 and (c == (r["iterations"] >> 0) + 2).all() and (o != 7.0).any()          # the same arrays, good arguments
    hip = _Hip()
    try:
        n = 65
        d_rays, d_out, d_rec, d_pts, d_cnt = hip.alloc(n * 32), hip.alloc(n * 16), hip.alloc(n * 32 + 16), hip.alloc(n * 16 * 16 + 16), hip.alloc(n * 4 + 16)
        for d, nbytes in ((d_out, n * 16), (d_rec, n * 32 + 16), (d_pts, n * 16 * 16 + 16), (d_cnt, n * 4 + 16)):
            assert hip.hip.hipMemset(d, PATTERN, C.c_size_t(nbytes)) == 0
        src = np.ascontiguousarray(_rays()[:n])
        assert hip.hip.hipMemcpy(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D) == 0

        def dev(n=n, s=0, mp=16, out=d_out.value, rec=d_rec.value, pts=d_pts.value, cnt=d_cnt.value, rays=d_rays.value):
            return _code(lambda: rp.trace_rays_paths_device(rays, n, s, mp, out, rec, pts, cnt))

        cases = {"max_points 1": dev(mp=1), "stride_log2 17": dev(s=17), "n * max_points over the limit": dev(n=4097, mp=4096), "NULL results": dev(out=0),
                 "NULL records": dev(rec=0), "NULL points": dev(pts=0), "NULL counts": dev(cnt=0), "points + 4": dev(pts=d_pts.value + 4), "points + 8": dev(pts=d_pts.value + 8),
                 "records + 8": dev(rec=d_rec.value + 8), "counts + 2": dev(cnt=d_cnt.value + 2), "counts + 1": dev(cnt=d_cnt.value + 1)}
        assert all(rc == E_INVALID for rc in cases.values()), cases
        rp.sync()
        for d, nbytes in ((d_out, n * 16), (d_rec, n * 32 + 16), (d_pts, n * 16 * 16 + 16), (d_cnt, n * 4 + 16)):
            back = np.zeros(nbytes // 4, np.uint32)
            assert hip.hip.hipMemcpy(C.c_void_p(back.ctypes.data), d, C.c_size_t(nbytes), hip.D2H) == 0
            assert (back == PATTERN_WORD).all(), "a refused call touched a device array"
        rp.trace_rays_paths_device(d_rays.value, n, 0, 16, d_out.value, d_rec.value, d_pts.value, d_cnt.value + 4)      # counts need 4-byte alignment only
        rp.trace_rays_paths_device(d_rays.value, 0, 0, 16, d_out.value, d_rec.value, d_pts.value, d_cnt.value)
        rp.sync()
    finally:
        hip.close()


# ---- 9. the hosts -----------------------------------------------------------------------------------------
def test_ray_path_agrees_with_pick():
    w, h = 96, 54
    r = B.Renderer(B.ladder_from_base((w, h), 3, 1), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    seen = set()
    for x, y in ((w // 2, h // 2), (w // 2, 4), (0, 0), (w // 2 + 9, h // 2 + 1)):
        pick = r.pick(x, y)
        p = r.ray_path(x, y)
        assert {k: p[k] for k in pick} == pick, (x, y)
        path, its = p["path"], p["path_iterations"]
        assert path.shape == (pick["iterations"] + 2, 3) and path.dtype == np.float32 and its.shape == (path.shape[0],)
        assert its[0] == 0 and tuple(path[0]) == tuple(np.float32(r.camera.position)) and its[-1] == pick["iterations"]
        assert np.array_equal(its[:-1], np.arange(path.shape[0] - 1))
        if pick["hit"] == B.HIT_NONE:
            assert tuple(float(v) for v in path[-1]) == pick["position"]
        q = r.ray_path(x, y, stride_log2=4)
        assert q["path"].shape == ((pick["iterations"] >> 4) + 2, 3)
        assert np.array_equal(_bits(q["path"][:-1]), _bits(path[:-1][::16])) and np.array_equal(_bits(q["path"][-1]), _bits(path[-1]))
        seen.add(pick["hit"])
    assert len(seen) >= 2, "the pixels must not all end alike"
    with pytest.raises(ValueError):
        r.ray_path(w, 0)


def test_cpp_host_prints_a_path(tmp_path):
    """bhray_render --path X Y [--path-stride S]: the pick line of that pixel, then one line per point - as many as the count, and Renderer.ray_path's numbers for the same
    pixel of the same scene (the two hosts form the ray with the same binary32 arithmetic; %.9g round-trips a binary32)"""
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
    for (x, y), s in (((12, 7), 0), ((12, 1), 0), ((0, 0), 2)):
        r = subprocess.run(base + ["--path", str(x), str(y)] + (["--path-stride", str(s)] if s else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        at = lines.index("24x14")
        f = lines[at + 1].split()
        want = r2.ray_path(x, y, stride_log2=s)
        assert f[:3] == ["pick", str(x), str(y)], lines[at + 1]
        field = {t.split("=")[0]: t.split("=")[1] for t in f[3:] if "=" in t}
        assert int(field["iterations"]) == want["iterations"]
        rows = [ln.split() for ln in lines[at + 2:]]
        assert len(rows) == (want["iterations"] >> s) + 2 == want["path"].shape[0], (len(rows), want["iterations"])
        assert np.array_equal(np.array([int(q[0]) for q in rows], np.uint32), want["path_iterations"])
        got = np.array([[float(v) for v in q[1:4]] for q in rows], np.float64).astype(np.float32)
        assert np.array_equal(_bits(got), _bits(want["path"])), "the printed points are not Renderer.ray_path's"
    far = subprocess.run(base + ["--path", "99", "7"], capture_output=True, text=True, timeout=120)
    assert far.returncode == 1 and "outside the frame" in far.stderr
    assert subprocess.run(base + ["--path", "3", "4", "--path-stride", "17"], capture_output=True, text=True, timeout=120).returncode == 2
