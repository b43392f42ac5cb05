"""-m gpu: still cameras - the accumulation image as a panorama, a fisheye or through a thin lens (bhray_accum_set_camera).

  6. The generated records are the restatement's (tests/still_camera_ref.py) in every word; a cropped frame's records are the window of the whole level's.
  7. The mean is, to the bit, the NumPy sum and mean over the device's own trace results for the restatement's rays; the grouping of samples changes no word.
  8. Adaptive: mean, counts and reach are tests/accum_adaptive_ref.py's over the restatement's rays.
  9. The equirect still and the lens still against the oracle's trace_ray of every sample ray, at 2 * REL_TOL + (S + 1) * 2^-23.
 10. The default camera - NULL or the explicit struct - leaves every word of a still; the refusals; frames keep their bits across a camera change.
 11. The display read under the equirect camera; Renderer.render_still / save_still and bhray_render --still-camera.

The frames are tests/test_gpu_accum.py's: ladder_for_frame((40, 36), 3, 2) - 1 440 pixels, no multiple of 64, a window of its 40 x 37 last level, large enough for the
display pass - and the 33 x 32 single-level frame."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from bhusie_amd.cameras import StillCamera
from tests import accum_adaptive_ref as AR
from tests import accum_ref as A
from tests import common as T
from tests import post_ref as P
from tests import rays_ref as RR
from tests import still_camera_ref as SR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1)}
CAMERAS = {"pinhole": (StillCamera.pinhole(), SR.Still()),
           "equirect": (StillCamera.equirect(), SR.Still(SR.EQUIRECT)),
           "fisheye": (StillCamera.fisheye(3.4), SR.Still(SR.FISHEYE, fisheye_fov=3.4)),
           "lens": (StillCamera.pinhole(lens_radius=0.3, focus_distance=12.0), SR.Still(SR.PINHOLE, lens_radius=0.3, focus_distance=12.0))}
NOT_DEFAULT = [k for k in CAMERAS if k != "pinhole"]
# inside the disk's outer radius and above its plane, looking slightly down at the hole: the panorama and the fisheye hold the disk all round, the horizon and the sky;
# further out for the lens (tests 9 asserts the classes from the oracle)
NEAR = B.Camera(position=(0.0, 1.5, -6.0), forward=(0.0, -0.25, 1.0), fov=1.3)
LENS_CAM = B.Camera(position=(0.0, 2.0, -12.0), forward=(0.0, -0.16, 1.0), fov=1.3)
SCENE_CAM = {"pinhole": LENS_CAM, "equirect": NEAR, "fisheye": NEAR, "lens": LENS_CAM}
ADAPTIVE = AR.Params(2, 6, 2, 0.05, 0.01)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(cfg=None, **kw):
    rp = B.RayPass(cfg if cfg is not None else CFGS["40x36_of_a_ladder"](), **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*T.textures())
    return rp


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _npix(cfg):
    return int(cfg.frame_w) * int(cfg.frame_h)


def _accumulate(rp, groups):
    rp.accum_begin()
    for g in groups:
        rp.accum_add(g)
    return rp.accum_read()


def _trace(rp, rec):
    """the device's trace results for the records; an unusable record (a fisheye sample outside the circle) is left out of the call and entered as (0, 0, 0, -1)"""
    usable = (rec[:, 4:7] != 0.0).any(axis=1)
    out = np.zeros((rec.shape[0], 4), np.float32)
    out[:, 3] = -1.0
    out[usable] = rp.trace_rays(np.ascontiguousarray(rec[usable]))
    return out


# ---- 6. records ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NOT_DEFAULT)
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_generated_records_are_the_restatements(shape, kind):
    cam = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
    still, ref = CAMERAS[kind]
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=cam))
    rp.accum_set_camera(still)
    assert _npix(rp.cfg) % 64 != 0
    for s in (0, 1, 7, 65535):
        got, want = rp.accum_sample_rays(s), SR.sample_rays(cam.uniform(), rp.cfg, ref, s)
        assert got.shape == want.shape == (_npix(rp.cfg), 8)
        differ = int((_bits(got) != _bits(want)).sum())
        assert differ == 0, f"{kind} sample {s}: {differ} of {got.size} words differ from the restatement"
    if kind == "fisheye":
        zero = (rp.accum_sample_rays(1)[:, 4:7] == 0.0).all(axis=1)
        assert 0 < int(zero.sum()) < zero.size, "the frame must hold samples inside and outside the image circle"
    rp.accum_set_camera(None)
    assert np.array_equal(_bits(rp.accum_sample_rays(7)), _bits(A.sample_rays(cam, rp.cfg, 7))), "NULL restores the pinhole generator"


@pytest.mark.parametrize("kind", NOT_DEFAULT)
def test_a_cropped_frames_records_are_a_window_of_the_whole_levels(kind):
    cam = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
    still, _ = CAMERAS[kind]
    cropped = _ctx(CFGS["40x36_of_a_ladder"]())
    cfg = cropped.cfg
    lw, lh = cfg.sizes()[-1]
    assert (lw, lh) != (cfg.frame_w, cfg.frame_h)
    whole = _ctx(B.ladder_from_base((lw, lh), 3, 1))
    for rp in (cropped, whole):
        rp.set_uniforms(*T.uniforms(camera=cam))
        rp.accum_set_camera(still)
    for s in (0, 7):
        level = whole.accum_sample_rays(s).reshape(lh, lw, 8)
        window = level[cfg.crop_y:cfg.crop_y + cfg.frame_h, cfg.crop_x:cfg.crop_x + cfg.frame_w].reshape(-1, 8)
        assert np.array_equal(_bits(cropped.accum_sample_rays(s)), _bits(window)), f"{kind} sample {s}"


# ---- 7. accumulation, to the bit ----------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("kind", NOT_DEFAULT)
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_mean_is_the_numpy_sum_of_the_devices_own_results(shape, kind, method):
    S = 5
    cam = SCENE_CAM[kind]
    still, ref = CAMERAS[kind]
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=method))
    per_sample = [_trace(rp, SR.sample_rays(cam.uniform(), rp.cfg, ref, s)) for s in range(S)]
    total = A.accumulate(per_sample, T.textures()[2])
    want = A.mean(total)
    rp.accum_set_camera(still)
    got = _accumulate(rp, [S])
    assert rp.accum_samples() == S and got.shape == (rp.cfg.frame_h, rp.cfg.frame_w, 4)
    if kind == "fisheye":
        outside = np.stack([r[:, 3] == -1.0 for r in per_sample])
        assert outside.all(axis=0).any() and (outside.any(axis=0) & ~outside.all(axis=0)).any(), "pixels wholly outside the circle, and pixels on its rim"
        assert (total[outside.all(axis=0), 3] == S).all(), "a sample outside the circle is a black sample: it counts"
    differ = int((_bits(got.reshape(-1, 4)) != _bits(want)).sum())
    print(f"{shape} {kind} method {method}: {differ} of {want.size} words differ")
    assert differ == 0, f"{differ} of {want.size} words differ from the NumPy sum over the device's results"
    assert np.array_equal(_bits(_accumulate(rp, [2, 1, 2])), _bits(got)), "add(2); add(1); add(2) differs from add(5)"
    rp.accum_set_camera(None)
    assert not np.array_equal(_bits(_accumulate(rp, [S])), _bits(got)), "the camera must change the image"


# ---- 8. adaptive --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["equirect", "lens"])
def test_adaptive_stills_follow_the_camera(kind):
    p = ADAPTIVE
    cam = SCENE_CAM[kind]
    still, ref = CAMERAS[kind]
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=1))
    results = [_trace(rp, SR.sample_rays(cam.uniform(), rp.cfg, ref, s)) for s in range(p.max_samples)]
    st = AR.State(_npix(rp.cfg))
    info, actives = AR.call(st, p, results, T.textures()[2])
    assert len(actives) >= 2 and len(np.unique(st.issued)) == 3, "the scene must leave pixels at 2, 4 and 6 samples"
    rp.accum_set_camera(still)
    rp.accum_begin()
    got_info = rp.accum_add_adaptive(**p.as_kwargs())
    assert got_info == info, (got_info, info)
    assert rp.accum_samples() == info["reach"] == 6
    assert np.array_equal(rp.accum_read_counts().reshape(-1), st.issued)
    differ = int((_bits(rp.accum_read().reshape(-1, 4)) != _bits(AR.mean(st))).sum())
    assert differ == 0, f"{kind}: {differ} words of the adaptive mean differ from the restatement"
    rp.accum_set_launch_rays(_npix(rp.cfg) // 3)                  # the rounds cut into several launches: the same words
    rp.accum_begin()
    rp.accum_add_adaptive(**p.as_kwargs())
    assert np.array_equal(_bits(rp.accum_read().reshape(-1, 4)), _bits(AR.mean(st)))


# ---- 9. oracle ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_samples(kind, method, S):
    cfg = CFGS["40x36_of_a_ladder"]()
    cam, ref = SCENE_CAM[kind], CAMERAS[kind][1]
    sc = T.oracle_scene(*T.uniforms(camera=cam, integration_method=method), T.textures())
    out = []
    for s in range(S):
        rec = SR.sample_rays(cam.uniform(), cfg, ref, s)
        res, disk = RR.oracle_rays(sc, rec)
        out.append((rec, res, disk))
    return out


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("kind", ["equirect", "lens"])
def test_the_still_against_the_oracle(kind, method):
    S = 3
    samples = _oracle_samples(kind, method, S)
    per_sample = [r for _, r, _ in samples]
    assert all(np.isfinite(r).all() for r in per_sample), "the oracle's samples are finite"
    rec, res, disk = samples[0]
    n_disk = int((disk > 0).sum())
    n_horizon = int(((res[:, 3] == 1.0) & (disk == 0) & (res[:, 0:3] == 0.0).all(axis=1)).sum())
    n_escape = int((res[:, 3] == 0.0).sum())
    assert n_disk >= 10 and n_horizon >= 10 and n_escape >= 10, (n_disk, n_horizon, n_escape)
    if kind == "lens":
        origins = np.unique(_bits(rec[:, 0:3]), axis=0)
        assert len(origins) > rec.shape[0] // 2, "the rays of a lens still start at differing origins"
        off = rec[:, 0:3].astype(np.float64) - np.frombuffer(SCENE_CAM[kind].uniform(), np.float32)[0:3]
        r = np.linalg.norm(off, axis=1)
        assert r.max() > 0.2 and r.min() < 0.1 and r.max() <= 0.3 * (1 + 1e-5), "origins across the aperture"
    want = A.mean(A.accumulate(per_sample, T.textures()[2]))
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=SCENE_CAM[kind], integration_method=method))
    rp.accum_set_camera(CAMERAS[kind][0])
    got = _accumulate(rp, [S]).reshape(-1, 4)
    assert np.array_equal(got[:, 3], want[:, 3])
    bar = 2 * T.REL_TOL + (S + 1) * 2.0 ** -23                    # tests/test_gpu_accum.py's bar, for the reasons given there
    err = float(T.rel_err(got[:, 0:3], want[:, 0:3]).max())
    print(f"{kind} method {method}: max rel err {err:.3g} (bar {bar:.3g}); disk {n_disk}, horizon {n_horizon}, escape {n_escape} rays in sample 0; "
          f"bit-identical {100.0 * float((_bits(got) == _bits(want)).all(axis=1).mean()):.2f} %")
    assert err <= bar, f"max rel err {err:.3g} > {bar:.3g}"


# ---- 10. the default, the refusals, frames ------------------------------------------------------------
def test_the_default_camera_changes_no_word():
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=LENS_CAM, integration_method=1))
    plain = _accumulate(rp, [5])
    rays = rp.accum_sample_rays(3)
    rp.accum_set_camera(None)
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(plain)) and np.array_equal(_bits(rp.accum_sample_rays(3)), _bits(rays))
    rp.accum_set_camera(StillCamera())                            # the explicit default struct
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(plain)) and np.array_equal(_bits(rp.accum_sample_rays(3)), _bits(rays))
    rp.accum_set_camera(StillCamera.pinhole(lens_radius=0.0, focus_distance=float("nan")))      # no lens: the focus is not read
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(plain))
    rp.accum_set_camera(StillCamera.equirect())
    assert not np.array_equal(_bits(_accumulate(rp, [5])), _bits(plain))
    rp.accum_set_camera(None)
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(plain)), "NULL restores the default"


def test_refusals_leave_the_camera_in_force():
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=NEAR, integration_method=1))
    rp.accum_set_camera(StillCamera.equirect())
    rays = rp.accum_sample_rays(1)
    L, h = rp._L, rp._h
    import ctypes as C

    def bad(**kw):
        s = StillCamera().struct()
        for k, v in kw.items():
            setattr(s, k, v)
        rc = L.bhray_accum_set_camera(h, C.byref(s))
        if rc != 0:
            assert L.bhray_last_error(h), "a refusal carries a message"
            assert np.array_equal(_bits(rp.accum_sample_rays(1)), _bits(rays)), f"a refused camera changed the state: {kw}"
        return rc
    assert bad(struct_size=16) == E_INVALID and bad(projection=3) == E_INVALID
    for fov in (0.0, -1.0, 6.3, float("nan"), float("inf")):
        assert bad(projection=2, fisheye_fov=fov) == E_INVALID, fov
    for r in (-0.5, float("nan"), float("inf")):
        assert bad(lens_radius=r) == E_INVALID, r
    assert bad(projection=1, lens_radius=0.1, focus_distance=5.0) == E_INVALID and bad(projection=2, fisheye_fov=2.0, lens_radius=0.1, focus_distance=5.0) == E_INVALID
    for f in (0.0, -2.0, float("nan"), float("inf")):
        assert bad(lens_radius=0.1, focus_distance=f) == E_INVALID, f
    assert _code(lambda: rp.accum_set_camera(StillCamera.fisheye(7.0))) == E_INVALID
    assert bad(projection=2, fisheye_fov=6.28318548) == 0         # accepted: 2 pi itself
    # every refusal of bhray_accum_add stays on bhray_accum_add, with a camera set
    u = T.uniforms(camera=NEAR, integration_method=1)
    rp.accum_set_camera(StillCamera.equirect())
    fresh = _ctx()
    fresh.accum_set_camera(StillCamera.equirect())                # accepted before begin and before the uniforms
    assert _code(lambda: fresh.accum_add(1)) == E_STATE
    fresh.accum_begin()
    assert _code(lambda: fresh.accum_add(1)) == E_STATE
    rp.accum_begin()
    rp.set_mesh_lensing(True)
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    rp.set_mesh_lensing(False)
    rp.accum_add(1)
    for kw in ({"literal": True}, {"eval_fma": True}, {"devices": [0, 0]}, {"row_rank": 0, "row_world": 2}):
        q = _ctx(**kw)
        q.set_uniforms(*u)
        q.accum_set_camera(StillCamera.equirect())                # validates and stores: accepted
        assert _code(q.accum_begin) == E_STATE, kw
        assert _code(lambda: q.accum_add(1)) == E_STATE, kw


def test_frames_keep_their_bits_across_a_camera_change():
    u = T.uniforms(camera=NEAR, integration_method=1)
    rp = _ctx()
    rp.set_uniforms(*u)
    rp.render()
    frame = rp.read_hdr().copy()
    rp.accum_set_camera(StillCamera.fisheye(3.4))
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed with the still camera"
    still = _accumulate(rp, [3])
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed behind a fisheye still"
    rp.accum_set_camera(StillCamera.pinhole(lens_radius=0.3, focus_distance=6.0))
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame))
    rp.accum_set_camera(StillCamera.fisheye(3.4))
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(still))


# ---- 11. display and hosts ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_display_read_under_the_equirect_camera(shape):
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=NEAR, integration_method=1))
    rp.accum_set_camera(StillCamera.equirect())
    mean = _accumulate(rp, [4])
    disp = rp.accum_read_display()
    with np.errstate(over="ignore"):
        sky16 = mean.astype(np.float16)                           # nearest even
    assert np.array_equal(disp, P.post_ref(sky16)), "the display read differs from post_ref over the binary16 mean"
    assert np.array_equal(_bits(rp.accum_read()), _bits(mean)), "the display read changed the mean"


def test_render_still_and_save_still_take_the_camera(tmp_path):
    r = B.Renderer(CFGS["40x36_of_a_ladder"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    r.camera = NEAR
    still = r.render_still(samples=4, camera=StillCamera.equirect())
    rp = _ctx()
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    rp.accum_set_camera(StillCamera.equirect())
    want = _accumulate(rp, [4])
    assert np.array_equal(_bits(still), _bits(want))
    plain = r.render_still(samples=4)                             # camera=None: the pinhole again
    rp.accum_set_camera(None)
    assert np.array_equal(_bits(plain), _bits(_accumulate(rp, [4]))) and not np.array_equal(_bits(plain), _bits(still))
    lens = StillCamera.pinhole(lens_radius=0.3, focus_distance=6.0)
    blurred = r.render_still(samples=4, shutter=2.0, camera=lens)
    det = B.RayDetails(integration_method=1)
    rp.accum_set_camera(lens)
    rp.accum_begin()
    for s in range(4):                                            # the shutter's loop with the lens in force
        det.time = r.ray_details.time + 2.0 * s / 4
        rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), det.uniform())
        rp.accum_add(1)
    assert np.array_equal(_bits(blurred), _bits(rp.accum_read()))
    p = ADAPTIVE
    adaptive = r.render_still(adaptive=B.AdaptiveStill(**p.as_kwargs()), camera=StillCamera.equirect())
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    rp.accum_set_camera(StillCamera.equirect())
    rp.accum_begin()
    assert rp.accum_add_adaptive(**p.as_kwargs()) == r.still_info
    assert np.array_equal(_bits(adaptive), _bits(rp.accum_read()))
    from PIL import Image
    path = tmp_path / "still.png"
    r.save_still(path, samples=4, camera=StillCamera.equirect())
    rp.accum_set_camera(StillCamera.equirect())
    _accumulate(rp, [4])
    want8 = rp.accum_read_display()
    want8[..., 3] = 255
    assert np.array_equal(np.asarray(Image.open(path).convert("RGBA")), want8)


@pytest.mark.parametrize("args, still", [(["--still-camera", "equirect"], StillCamera.equirect()), (["--still-camera", "fisheye", "3.4"], StillCamera.fisheye(3.4)),
                                         (["--lens", "0.25", "19"], StillCamera.pinhole(lens_radius=0.25, focus_distance=19.0))], ids=["equirect", "fisheye", "lens"])
def test_cpp_host_writes_a_still_with_the_camera(tmp_path, args, still):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "still.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp", "4"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "40x37"
    got = np.fromfile(out, dtype=np.float32).reshape(37, 40, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    assert np.array_equal(_bits(got), _bits(r2.render_still(samples=4, camera=still))), "the C++ host's still differs from the Python host's"
    assert not np.array_equal(_bits(got), _bits(r2.render_still(samples=4)))
