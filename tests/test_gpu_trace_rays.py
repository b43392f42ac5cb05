"""-m gpu: caller-supplied ray batches (bhray_trace_rays, bhray_trace_rays_device).

  1. create_ray's rays through trace_rays = the `levels = 1` frame, bit for bit (both integrators; the default scene, the camera inside the sphere, the hole away from the
     origin, a mesh in flat space): integrator, shading, traversal and epilogue of the ray-list kernels are the shipped kernels'.
  2. 4 133 rays of arbitrary origin against oracle.trace_ray at the bars of tests/test_gpu_parity.py: no alpha mismatch, escape directions to the bit, colours within 1e-4.
  3. n = 0, 1, 63, 64, 65: a ray's result does not depend on its batch.       4. The device variant on a stream of the caller's; unusable rays.
  5. Frames before and after a batch keep their bits; a model upload waits for an outstanding batch; the refused states.       6. A panorama through Renderer.render_rays."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras
from oracle import oracle as O
from tests import common as T
from tests import rays_ref as RR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
W, H = 96, 54


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(cfg=None, **kw):
    rp = B.RayPass(cfg if cfg is not None else B.ladder_from_base((24, 14), 3, 1), **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*T.textures())
    return rp


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


# ---- 1. pixel rays reproduce the frame ---------------------------------------------------------------
INSIDE = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
FAR = B.Camera(position=(2.0, 1.0, -45.0), forward=(0.0, 0.0, 1.0), fov=0.9)
MESH_CAM = B.Camera(position=(0.0, 0.0, -60.0), forward=(-0.1, 0.0, 1.0), fov=1.0)
MESH_AT = (-22.0, 4.0, -25.0)              # outside the sphere, 41 in front of MESH_CAM: about 190 of the 5 184 pixels (counted with the oracle)
# The hole away from the origin, and a disk whose outer radius (26) lies beyond |hole| + the sphere's radius (2.6 + 20).  The shader's disk density is
# 1 - |ip| / outer with ip the hit's ABSOLUTE position (ray.wgsl:616), so with the default outer radius (10) a hit near the rim on the side away from the origin has a
# negative density, pow(negative, 1.3) is a NaN and so is the pixel's colour: 16-18 pixels of this 96 x 54 frame, by the oracle.  A NaN's sign and payload are not
# specified by IEEE 754 (6.2, 6.3) and on gfx950 follow instruction selection (a source negation modifier flips a NaN operand's sign bit), so two builds of one source
# text may differ in them: with outer = 10 one such pixel of the RK frame came out 0xffc00000 from the frame's kernel and 0x7fc00000 from the ray-list kernel (measured;
# tests/common.assert_parity leaves non-finite pixels out for the same reason).  Bits can only be demanded where the arithmetic defines them: the disk here reaches
# beyond the sphere, every hit has |ip| < outer, and the test asserts that the frame is finite before it compares all of its words.
HOLE_AWAY = B.BlackHole(position=(1.5, -0.75, 2.0), accretion_disk_outer=26.0)
PIXEL_SCENES = {
    "default": (B.Camera(), B.BlackHole(), False),
    "camera_inside_the_sphere": (INSIDE, B.BlackHole(), False),
    "hole_away_from_the_origin": (FAR, HOLE_AWAY, False),
    "mesh_in_flat_space": (MESH_CAM, B.BlackHole(), True),
}


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("scene", list(PIXEL_SCENES))
def test_pixel_rays_reproduce_the_frame_bit_for_bit(scene, method):
    cam, bh, mesh = PIXEL_SCENES[scene]
    rp = _ctx(B.ladder_from_base((W, H), 3, 1))                   # levels = 1: every pixel is traced
    if mesh:
        rp.upload_model(RR.mesh_model(MESH_AT))
    rp.set_uniforms(*T.uniforms(camera=cam, black_hole=bh, integration_method=method, model_count=1 if mesh else 0))
    rp.render()
    frame = rp.read_hdr()
    assert frame.shape == (H, W, 4)
    assert np.isfinite(frame).all(), "a scene of this test must not produce NaN pixels: their bits are not defined (see HOLE_AWAY)"
    assert len(np.unique(frame[..., 3])) == 2, "both pixel classes"
    got = rp.trace_rays(cameras.pinhole_rays(cam, W, H)).reshape(H, W, 4)
    differ = int((_bits(got) != _bits(frame)).sum())
    print(f"{scene} method {method}: {differ} of {frame.size} words differ; classes {np.unique(frame[..., 3], return_counts=True)}")
    assert differ == 0, f"{differ} of {frame.size} words differ from the frame"
    if scene == "camera_inside_the_sphere":
        assert float(np.linalg.norm(np.array(cam.position) - np.array(bh.position))) < bh.relativity_sphere_radius
    if mesh:                                                      # the comparison is about a mesh only if the frame shows it
        rp.set_uniforms(*T.uniforms(camera=cam, black_hole=bh, integration_method=method, model_count=0))
        rp.render()
        assert int((_bits(rp.read_hdr()) != _bits(frame)).any(axis=2).sum()) >= 50, "the mesh covers too few pixels of the frame"


# ---- 2. arbitrary origins against the oracle --------------------------------------------------------
def _assert_ray_parity(got, want, what):
    """tests/test_gpu_parity.py's bars: 0 alpha mismatches, alpha-0 directions bit-identical, colours within 1e-4 relative"""
    assert got.shape == want.shape
    alpha = int((got[:, 3] != want[:, 3]).sum())
    esc = want[:, 3] == 0.0
    dirs = int((_bits(got[esc]) != _bits(want[esc])).any(axis=1).sum())
    err = float(T.rel_err(got[~esc], want[~esc]).max(initial=0.0))
    print(f"{what}: {alpha} alpha mismatches, {dirs} of {int(esc.sum())} escape directions differ, max rel colour err {err:.3g}, "
          f"bit-identical {100.0 * float((_bits(got) == _bits(want)).all(axis=1).mean()):.2f} %")
    assert alpha == 0, f"{what}: {alpha} alpha mismatches"
    assert dirs == 0, f"{what}: {dirs} escape directions differ from the oracle's bits"
    assert err <= T.REL_TOL, f"{what}: max rel err {err:.3g} > {T.REL_TOL}"


def _gpu_results(method, mesh=False):
    rp = _ctx()
    if mesh:
        rp.upload_model(RR.mesh_model())
    rp.set_uniforms(*RR.scene_uniforms(method, 1 if mesh else 0))
    return rp, rp.trace_rays(RR.seeded_rays())


@pytest.mark.parametrize("method,mesh", [(0, False), (1, False), (1, True)], ids=["euler", "rk", "rk_mesh"])
def test_arbitrary_origins_match_the_oracle(method, mesh):
    rec, want, disk = RR.reference(method, mesh)
    counts = RR.class_counts(rec, want, disk)
    print(counts)
    assert rec.shape[0] == 4133 and min(counts.values()) >= RR.MIN_PER_CLASS, f"the comparison needs every outcome: {counts}"
    if mesh:
        assert int((RR.reference(method, False)[1] != want).any(axis=1).sum()) >= 20, "the mesh changes too few rays"
    _, got = _gpu_results(method, mesh)
    _assert_ray_parity(got, want, f"method {method} mesh {mesh}")


# ---- 3. sizes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_a_rays_result_does_not_depend_on_its_batch(method):
    rec = RR.seeded_rays()
    rp, full = _gpu_results(method)
    for n in (0, 1, 63, 64, 65):
        got = rp.trace_rays(rec[:n])
        assert got.shape == (n, 4)
        assert np.array_equal(_bits(got), _bits(full[:n])), f"n = {n}: differs from the prefix of the full batch"
    six = rec[:65][:, [0, 1, 2, 4, 5, 6]]                           # the (n, 6) form is the same rays
    assert np.array_equal(_bits(rp.trace_rays(six)), _bits(full[:65]))


# ---- 4. the device variant --------------------------------------------------------------------------
class _Hip:
    H2D, D2H = 1, 2

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        assert self.hip.hipSetDevice(0) == 0
        self.stream = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(self.stream), 1) == 0          # hipStreamNonBlocking: ordered against nothing but what the test enqueues
        self.allocs = []

    def alloc(self, nbytes):
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), C.c_size_t(max(nbytes, 16))) == 0
        self.allocs.append(d)
        return d

    def close(self):
        assert self.hip.hipStreamSynchronize(self.stream) == 0
        for d in self.allocs:
            self.hip.hipFree(d)
        self.hip.hipStreamDestroy(self.stream)


def _with_unusable_rays(rec):
    """the list with four special records among it: a NaN origin, an Inf direction, a zero direction (unusable) and a NaN pad with good components (traced)"""
    r = rec.copy()
    bad = {"nan_origin": 7, "inf_direction": 64, "zero_direction": 1000, "nan_pad": 129}
    r[bad["nan_origin"], 1] = np.nan
    r[bad["inf_direction"], 6] = np.inf
    r[bad["zero_direction"], 4:7] = 0.0
    r[bad["nan_pad"], 3] = np.nan; r[bad["nan_pad"], 7] = np.nan
    return r, bad


def test_device_variant_on_a_callers_stream_and_unusable_rays():
    rec = RR.seeded_rays()
    n = rec.shape[0]
    rp, host = _gpu_results(1)
    special, bad = _with_unusable_rays(rec)
    hip = _Hip()
    try:
        d_rays, d_out = hip.alloc(n * 32), hip.alloc(n * 16)
        src = np.ascontiguousarray(special)
        # rays in, trace, results out: all on the caller's stream, one synchronisation at the very end
        assert hip.hip.hipMemcpyAsync(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D, hip.stream) == 0
        assert hip.hip.hipMemsetAsync(d_out, 0xFF, C.c_size_t(n * 16), hip.stream) == 0
        rp.trace_rays_device(d_rays.value, n, d_out.value, stream=hip.stream.value)
        got = np.zeros((n, 4), dtype=np.float32)
        assert hip.hip.hipMemcpyAsync(C.c_void_p(got.ctypes.data), d_out, C.c_size_t(got.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipStreamSynchronize(hip.stream) == 0
        rp.sync()
        unusable = [bad["nan_origin"], bad["inf_direction"], bad["zero_direction"]]
        for k in unusable:
            assert got[k].tolist() == [0.0, 0.0, 0.0, -1.0], (k, got[k])
        keep = np.ones(n, dtype=bool); keep[unusable] = False
        differ = int((_bits(got[keep]) != _bits(host[keep])).any(axis=1).sum())
        assert differ == 0, f"{differ} results differ from the host variant's (the pad ray and the unusable rays' neighbours among them)"
        assert np.array_equal(_bits(got[bad["nan_pad"]]), _bits(host[bad["nan_pad"]])) and host[bad["nan_pad"], 3] in (0.0, 1.0)
        # the host variant refuses the same list as a whole and leaves the output alone
        out = np.full((n, 4), 7.0, dtype=np.float32)
        L = B.lib()
        rc = L.bhray_trace_rays(rp._h, src.ctypes.data_as(C.POINTER(B.BhrayRay)), n, out.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == E_INVALID and (out == 7.0).all()
        # n == 0 and the argument checks
        rp.trace_rays_device(d_rays.value, 0, d_out.value, stream=hip.stream.value)
        assert _code(lambda: rp.trace_rays_device(0, 5, d_out.value)) == E_INVALID
        assert _code(lambda: rp.trace_rays_device(d_rays.value, (1 << 26) + 1, d_out.value)) == E_INVALID
    finally:
        hip.close()


# ---- 5. coexistence ---------------------------------------------------------------------------------
def test_frames_before_and_after_a_batch_keep_their_bits():
    cfg = B.ladder_from_base((40, 24), 3, 2)
    cams = [B.Camera(position=(0.0, 0.0, -19.0)), B.Camera(position=(1.0, 0.5, -30.0), forward=(0.0, 0.05, 1.0))]

    def run(with_batch):
        rp = _ctx(cfg, frames_in_flight=4)
        rows, width = len(rp.local_rows()), rp.frame_size[0]
        first = B.PinnedFrame(rows, width)
        rp.set_uniforms(*T.uniforms(camera=cams[0], integration_method=1))
        rp.render()
        ticket = rp.read_hdr_async(first)                         # in stream order behind the first frame: nothing waits here
        batch = rp.trace_rays(RR.seeded_rays()[:1000]) if with_batch else None
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
        assert np.array_equal(_bits(plain[k]), _bits(mixed[k])), f"frame {k} changed with a ray batch between the renders"
    assert np.array_equal(_bits(batch), _bits(_gpu_results(1)[1][:1000])), "the batch between two frames differs from the batch alone"


def test_a_model_upload_waits_for_an_outstanding_batch():
    rec = RR.seeded_rays()
    n = rec.shape[0]
    old, new = RR.mesh_model(), RR.mesh_model((0.0, -30.0, 5.0))
    rp = _ctx()
    rp.upload_model(old)
    rp.set_uniforms(*RR.scene_uniforms(1, 1))
    want_old = rp.trace_rays(rec)
    hip = _Hip()
    try:
        d_rays, d_out = hip.alloc(n * 32), hip.alloc(n * 16)
        src = np.ascontiguousarray(rec)
        assert hip.hip.hipMemcpy(d_rays, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), hip.H2D) == 0
        rp.trace_rays_device(d_rays.value, n, d_out.value, stream=hip.stream.value)
        rp.upload_model(new)                                      # with the batch outstanding: must wait for it, not pull the old model from under it
        got = np.zeros((n, 4), dtype=np.float32)
        assert hip.hip.hipMemcpyAsync(C.c_void_p(got.ctypes.data), d_out, C.c_size_t(got.nbytes), hip.D2H, hip.stream) == 0
        assert hip.hip.hipStreamSynchronize(hip.stream) == 0
        assert np.array_equal(_bits(got), _bits(want_old)), "the outstanding batch did not see the OLD model"
        want_new = rp.trace_rays(rec)
        assert int((_bits(want_new) != _bits(want_old)).any(axis=1).sum()) >= 20, "the two models must differ in the rays' results"
        rp.sync()
    finally:
        hip.close()


def test_refused_states():
    rec = RR.seeded_rays()[:65]
    u = RR.scene_uniforms(1)
    rp = _ctx()
    assert _code(lambda: rp.trace_rays(rec)) == E_STATE           # before the first set_uniforms
    rp.set_uniforms(*u)
    assert rp.trace_rays(rec).shape == (65, 4)
    for kw in ({"literal": True}, {"eval_fma": True}):           # no such kernels
        q = _ctx(**kw)
        q.set_uniforms(*u)
        assert _code(lambda: q.trace_rays(rec)) == E_STATE, kw
    rp.set_mesh_lensing(True)                                    # out of scope here
    assert _code(lambda: rp.trace_rays(rec)) == E_STATE
    rp.set_mesh_lensing(False)
    assert rp.trace_rays(rec).shape == (65, 4)
    multi = _ctx(devices=[0, 0])                                 # a multi-device ctx (the same device listed twice)
    multi.set_uniforms(*u)
    assert _code(lambda: multi.trace_rays(rec)) == E_STATE
    assert _code(lambda: rp.trace_rays(np.full((1, 6), np.nan, np.float32))) == E_INVALID
    counting = _ctx(counters=True)                               # runs the kernels that do not count: its counters do not move
    counting.set_uniforms(*u)
    counting.render(); counting.sync()
    before = counting.counters()
    assert np.array_equal(_bits(counting.trace_rays(rec)), _bits(rp.trace_rays(rec)))
    assert counting.counters() == before


# ---- 6. panorama ------------------------------------------------------------------------------------
def test_panorama_through_render_rays():
    pw, ph = 64, 32
    r = B.Renderer(B.ladder_from_base((24, 14), 3, 1), device=0)
    tex = T.textures()
    r.ray_pass.set_textures(*tex)
    r.ray_details.integration_method = 1
    position, forward = (4.0, -3.0, -26.0), (0.0, 0.1, 1.0)
    rays = cameras.equirect_rays(position, forward, pw, ph)
    img = r.render_rays(rays, (ph, pw))
    assert img.shape == (ph, pw, 4) and img.dtype == np.float32
    sc = T.oracle_scene(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform(), tex)
    want, _ = RR.oracle_rays(sc, rays)
    assert len(np.unique(want[:, 3])) == 2, "the panorama must show both pixel classes"
    _assert_ray_parity(img.reshape(-1, 4), want, "panorama")
    sky = r.render_rays(rays, (ph, pw), resolve_sky=True)
    assert sky.shape == (ph, pw, 4) and sky.dtype == np.float16
    want_sky = O.sky_resolve(img, tex[2])
    assert np.array_equal(sky.view(np.uint16), want_sky.view(np.uint16)), "the sky pass over the rays' image differs from oracle_sky_resolve of that image"
    # a fisheye's pixels outside its circle are not traced: alpha -1, black, also through the sky pass
    fr = cameras.fisheye_rays(position, forward, 33, 33, 3.0)
    fimg, fsky = r.render_rays(fr, (33, 33)), r.render_rays(fr, (33, 33), resolve_sky=True)
    outside = (fr[:, 4:7] == 0.0).all(axis=1).reshape(33, 33)
    assert outside[0, 0] and not outside[16, 16]
    assert (fimg[outside] == np.array([0, 0, 0, -1], np.float32)).all() and (fsky[outside] == np.array([0, 0, 0, -1], np.float16)).all()
    assert np.isin(fimg[~outside][:, 3], (0.0, 1.0)).all() and (fsky[~outside][:, 3] == 1.0).all()


def test_cpp_host_writes_a_panorama(tmp_path):
    """bhray_render --panorama W H: the same image as Renderer.render_rays over cameras.equirect_rays, up to the last bits of the two hosts' sin / cos (a ray that grazes
    an outcome's boundary may fall on the other side): the classes of nearly all pixels, and the file the existing output path writes."""
    import os
    import subprocess
    from bhusie_amd import assets
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "pano.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "24", "14", "--levels", "1", "--disk-size", "64", "--panorama", "48", "24"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "48x24"
    got = np.fromfile(out, dtype=np.float32)
    assert got.size == 48 * 24 * 4
    got = got.reshape(24, 48, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)                                # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((24, 14), 3, 1), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    want = r2.render_rays(cameras.equirect_rays(r2.camera.position, r2.camera.forward, 48, 24), (24, 48))
    assert np.isin(got[..., 3], (0.0, 1.0)).all() and len(np.unique(got[..., 3])) == 2
    same = float((got[..., 3] == want[..., 3]).mean())
    close = float((np.abs(got - want).max(axis=2) <= 1e-3).mean())
    print(f"classes equal on {100 * same:.2f} %, values within 1e-3 on {100 * close:.2f} % of the pixels")
    assert same >= 0.98 and close >= 0.9
