"""-m gpu: supersampled stills - the accumulation image (bhray_accum_*).

  1. The generator's rays are the restatement's (tests/accum_ref.py) in every word; sample 0 is create_ray's pixel-centre ray.
  2. The mean is, to the bit, the NumPy sum and mean over the device's own trace results for the restatement's rays; one sample is the resolved `levels = 1` frame.
  3. The grouping of samples into calls and launches does not change a word; begin clears.
  4. The mean against the oracle's trace_ray of every sample, at 2 * REL_TOL + (S + 1) * 2^-23.
  5. Samples whose colour is not finite are skipped: the mean stays finite and divides by the samples taken.
  6. The display read is tests/post_ref.py over the binary16 rounding of the mean, byte for byte.
  7. The refused states; frames keep their bits; a model upload waits for an outstanding accumulation; the cap.
  8. Renderer.render_still / save_still and bhray_render --spp.

The frame is ladder_for_frame((40, 36), 3, 2) - 1 440 pixels: no multiple of 64 or 256, a frame that is a window of its last level (40 x 37), large enough for the
display pass - and one 33 x 32 single-level frame."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, cameras
from tests import accum_ref as A
from tests import common as T
from tests import post_ref as P
from tests import rays_ref as RR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1)}
CAM = B.Camera()                                                  # the default scene: the hole at the origin, so no NaN pixels (asserted from the oracle in 4.)
# tests/test_gpu_trace_rays.py's hole-away scene with the default disk: the far rim's hits have a negative density, pow(negative, 1.3) is a NaN colour
FAR = B.Camera(position=(2.0, 1.0, -45.0), forward=(0.0, 0.0, 1.0), fov=0.9)
HOLE_AWAY_NAN = B.BlackHole(position=(1.5, -0.75, 2.0))
MESH_CAM = B.Camera(position=(0.0, 0.0, -60.0), forward=(-0.1, 0.0, 1.0), fov=1.0)
MESH_AT = (-22.0, 4.0, -25.0)


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


def _restated_mean(rp, cam, S):
    """the NumPy sum and mean over the DEVICE's trace results for the restatement's rays of samples 0 .. S-1; also the samples each pixel took"""
    per_sample = [rp.trace_rays(A.sample_rays(cam, rp.cfg, s)) for s in range(S)]
    total = A.accumulate(per_sample, T.textures()[2])
    return A.mean(total), total[:, 3]


# ---- 1. rays ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_generated_rays_are_the_restatements(shape):
    cam = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=cam))
    cfg = rp.cfg
    assert _npix(cfg) % 64 != 0
    for s in (0, 1, 7):
        got, want = rp.accum_sample_rays(s), A.sample_rays(cam, cfg, s)
        assert got.shape == want.shape == (_npix(cfg), 8)
        differ = int((_bits(got) != _bits(want)).sum())
        assert differ == 0, f"sample {s}: {differ} of {got.size} words differ from the restatement"
    lw, lh = cfg.sizes()[-1]
    level = cameras.pinhole_rays(cam, lw, lh).reshape(lh, lw, 8)
    window = level[cfg.crop_y:cfg.crop_y + cfg.frame_h, cfg.crop_x:cfg.crop_x + cfg.frame_w].reshape(-1, 8)
    assert np.array_equal(_bits(rp.accum_sample_rays(0)), _bits(window)), "sample 0 is not create_ray's ray of the pixel"
    assert not np.array_equal(_bits(rp.accum_sample_rays(1)), _bits(window))
    assert _code(lambda: rp.accum_sample_rays(65536)) == E_INVALID


# ---- 2. accumulation, to the bit ----------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_mean_is_the_numpy_sum_of_the_devices_own_results(shape, method):
    S = 5
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method))
    want, n = _restated_mean(rp, CAM, S)
    got = _accumulate(rp, [S])
    assert rp.accum_samples() == S
    assert got.shape == (rp.cfg.frame_h, rp.cfg.frame_w, 4) and got.dtype == np.float32
    assert (n == S).all() and (got[..., 3] == 1.0).all()
    differ = int((_bits(got.reshape(-1, 4)) != _bits(want)).sum())
    print(f"{shape} method {method}: {differ} of {want.size} words differ")
    assert differ == 0, f"{differ} of {want.size} words differ from the NumPy sum over the device's results"


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_one_sample_is_the_resolved_single_level_frame(shape, method):
    rp = _ctx(CFGS[shape]())
    cfg = rp.cfg
    u = T.uniforms(camera=CAM, integration_method=method)
    rp.set_uniforms(*u)
    got = _accumulate(rp, [1])
    lw, lh = cfg.sizes()[-1]
    one = _ctx(B.ladder_from_base((lw, lh), 3, 1))                # levels = 1: every pixel of the last level is traced
    one.set_uniforms(*u)
    one.render()
    frame = one.read_hdr()[cfg.crop_y:cfg.crop_y + cfg.frame_h, cfg.crop_x:cfg.crop_x + cfg.frame_w]
    assert np.isfinite(frame).all() and len(np.unique(frame[..., 3])) == 2, "both pixel classes, no NaN"
    want = A.resolve(frame.reshape(-1, 4), T.textures()[2])
    assert np.array_equal(_bits(got.reshape(-1, 4)), _bits(want)), "one sample differs from the binary32 sky resolve of the levels = 1 frame"


# ---- 3. grouping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_grouping_of_samples_changes_no_word(method):
    rp = _ctx()
    npix = _npix(rp.cfg)
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method))
    whole = _accumulate(rp, [5])
    assert np.array_equal(_bits(_accumulate(rp, [2, 3])), _bits(whole)), "add(2); add(3) differs from add(5)"
    assert np.array_equal(_bits(_accumulate(rp, [1, 0, 4])), _bits(whole))
    rp.accum_set_launch_rays(npix)                                # K = 1: five launches
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole)), "one sample per launch differs from five in one"
    rp.accum_set_launch_rays(2 * npix + 7)                        # K = 2: launches of 2, 2, 1
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole))
    rp.accum_set_launch_rays(1)                                   # fewer rays than a sample has: still K = 1
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole))
    rp.accum_set_launch_rays(0)
    assert rp.accum_samples() == 5
    rp.accum_begin()                                              # clears
    assert rp.accum_samples() == 0
    assert not rp.accum_read().any(), "begin leaves an empty image: n = 0 everywhere, so (0, 0, 0, 0)"
    assert not np.array_equal(_bits(_accumulate(rp, [4])), _bits(whole))


# ---- 4. oracle ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_samples(method, S):
    cfg = CFGS["40x36_of_a_ladder"]()
    tex = T.textures()
    sc = T.oracle_scene(*T.uniforms(camera=CAM, integration_method=method), tex)
    return [RR.oracle_rays(sc, A.sample_rays(CAM, cfg, s))[0] for s in range(S)]


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_mean_against_the_oracle(method):
    S = 4
    per_sample = _oracle_samples(method, S)
    assert all(np.isfinite(r).all() for r in per_sample), "the hole at the origin: the oracle's samples are finite"
    alphas = np.stack([r[:, 3] for r in per_sample])
    mixed = int(((alphas == 0).any(axis=0) & (alphas == 1).any(axis=0)).sum())
    assert mixed >= 1, "some pixel's footprint must hold colour and sky samples"
    want = A.mean(A.accumulate(per_sample, T.textures()[2]))
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method))
    got = _accumulate(rp, [S]).reshape(-1, 4)
    assert np.array_equal(got[:, 3], want[:, 3])
    # every sample's colour is within REL_TOL of max(|want|, floor) and colours are non-negative, so the mean's error is at most REL_TOL * (mean + floor)
    # <= 2 REL_TOL max(mean, floor); the S additions and the division round once each
    bar = 2 * T.REL_TOL + (S + 1) * 2.0 ** -23
    err = float(T.rel_err(got[:, 0:3], want[:, 0:3]).max())
    print(f"method {method}: max rel err {err:.3g} (bar {bar:.3g}), {mixed} pixels with both classes among their samples, "
          f"bit-identical {100.0 * float((_bits(got) == _bits(want)).all(axis=1).mean()):.2f} %")
    assert err <= bar, f"max rel err {err:.3g} > {bar:.3g}"


# ---- 5. skipped samples -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_samples_that_are_not_finite_are_skipped(method):
    S = 5
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=FAR, black_hole=HOLE_AWAY_NAN, integration_method=method))
    want, n = _restated_mean(rp, FAR, S)
    print(f"method {method}: samples taken per pixel {dict(zip(*np.unique(n, return_counts=True)))}")
    assert (n < S).any(), "the scene must produce samples that are not finite"
    got = _accumulate(rp, [S]).reshape(-1, 4)
    assert np.isfinite(got).all(), "a NaN sample reached the mean"
    assert np.array_equal(got[:, 3] == 0.0, n == 0)
    differ = int((_bits(got) != _bits(want)).sum())
    assert differ == 0, f"{differ} words differ from the mean over the samples each pixel took"


# ---- 6. display ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_display_read_is_post_ref_of_the_rounded_mean(shape):
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=1))
    mean = _accumulate(rp, [4])
    disp = rp.accum_read_display()
    assert disp.shape == (rp.cfg.frame_h, rp.cfg.frame_w, 4) and disp.dtype == np.uint8
    with np.errstate(over="ignore"):
        sky16 = mean.astype(np.float16)                           # nearest even
    assert np.array_equal(disp, P.post_ref(sky16)), "the display read differs from post_ref over the binary16 mean"
    assert np.array_equal(_bits(rp.accum_read()), _bits(mean)), "the display read changed the mean"
    small = _ctx(B.ladder_from_base((24, 14), 3, 1))              # below the display pass's 32 x 32
    small.set_uniforms(*T.uniforms())
    small.accum_begin(); small.accum_add(1)
    assert _code(small.accum_read_display) == E_INVALID
    assert small.accum_read().shape == (14, 24, 4)


# ---- 7. state -----------------------------------------------------------------------------------------
def test_refused_states_and_the_cap():
    u = T.uniforms(camera=CAM, integration_method=1)
    rp = _ctx()
    assert _code(lambda: rp.accum_add(1)) == E_STATE              # before begin
    assert _code(rp.accum_read) == E_STATE and _code(rp.accum_read_display) == E_STATE
    assert rp.accum_samples() == 0
    rp.accum_begin()
    assert _code(lambda: rp.accum_add(1)) == E_STATE              # before the first set_uniforms
    rp.set_uniforms(*u)
    rp.accum_add(0)                                               # nothing happens
    assert rp.accum_samples() == 0
    rp.accum_add(3)
    before = rp.accum_read()
    assert _code(lambda: rp.accum_add(65536 - 2)) == E_INVALID    # 3 + 65 534 > BHRAY_ACCUM_MAX_SAMPLES
    assert _code(lambda: rp.accum_add(2 ** 32 - 1)) == E_INVALID
    assert rp.accum_samples() == 3 and np.array_equal(_bits(rp.accum_read()), _bits(before)), "a refused add touched the sum"
    rp.set_mesh_lensing(True)                                     # out of scope
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    rp.set_mesh_lensing(False)
    rp.accum_add(1)
    assert rp.accum_samples() == 4
    for kw in ({"literal": True}, {"eval_fma": True}, {"devices": [0, 0]}, {"row_rank": 0, "row_world": 2}):
        q = _ctx(**kw)
        q.set_uniforms(*u)
        assert _code(q.accum_begin) == E_STATE, kw
        assert _code(lambda: q.accum_add(1)) == E_STATE, kw
        assert q.accum_samples() == 0


def test_frames_before_and_after_an_accumulation_keep_their_bits():
    u = T.uniforms(camera=CAM, integration_method=1)
    plain = _ctx()
    plain.set_uniforms(*u)
    plain.render()
    frame = plain.read_hdr().copy()
    alone = _accumulate(plain, [3])
    rp = _ctx()
    rp.set_uniforms(*u)
    rp.render()
    rp.accum_begin(); rp.accum_add(3)                             # behind a frame in flight
    rp.render()
    second = rp.read_hdr().copy()
    mixed = rp.accum_read()
    rp.render()
    assert np.array_equal(_bits(second), _bits(frame)) and np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed with an accumulation beside it"
    assert np.array_equal(_bits(mixed), _bits(alone)), "the accumulation between two frames differs from the accumulation alone"


def test_a_model_upload_waits_for_an_outstanding_accumulation():
    old, new = RR.mesh_model(MESH_AT), RR.mesh_model((0.0, -30.0, 5.0))
    rp = _ctx()
    rp.upload_model(old)
    rp.set_uniforms(*T.uniforms(camera=MESH_CAM, integration_method=1, model_count=1))
    want_old = _accumulate(rp, [3])
    rp.accum_begin()
    rp.accum_add(3)
    rp.upload_model(new)                                          # with the samples outstanding: must wait for them, not pull the old model from under them
    assert np.array_equal(_bits(rp.accum_read()), _bits(want_old)), "the outstanding accumulation did not see the OLD model"
    want_new = _accumulate(rp, [3])
    assert int((_bits(want_new) != _bits(want_old)).any(axis=2).sum()) >= 20, "the two models must differ in the image"
    rp.sync()


# ---- 8. hosts -----------------------------------------------------------------------------------------
def _renderer():
    r = B.Renderer(CFGS["40x36_of_a_ladder"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    r.ray_details.time = 0.5
    return r


def test_render_still_is_the_ray_pass_calls(tmp_path):
    r = _renderer()
    still = r.render_still(samples=4)
    assert still.shape == (36, 40, 4) and still.dtype == np.float32 and r.ray_pass.accum_samples() == 4
    rp = _ctx()
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    assert np.array_equal(_bits(still), _bits(_accumulate(rp, [4])))
    assert np.array_equal(_bits(r.render_still(samples=4, shutter=0.0)), _bits(still))
    blurred = r.render_still(samples=4, shutter=2.0)
    assert r.ray_details.time == 0.5, "the shutter must leave ray_details.time as it was"
    det = B.RayDetails(integration_method=1)
    rp.accum_begin()
    for s in range(4):                                            # the hand-written loop: sample s at time + shutter * s / samples
        det.time = 0.5 + 2.0 * s / 4
        rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), det.uniform())
        rp.accum_add(1)
    assert np.array_equal(_bits(blurred), _bits(rp.accum_read()))
    assert not np.array_equal(_bits(blurred), _bits(still)), "the disk turns with time: the shutter must change the image"
    from PIL import Image
    path = tmp_path / "still.png"
    r.save_still(path, samples=4)
    want = r.ray_pass.accum_read_display()
    want[..., 3] = 255
    assert np.array_equal(np.asarray(Image.open(path).convert("RGBA")), want)
    assert np.array_equal(_bits(r.ray_pass.accum_read()), _bits(still))


def test_cpp_host_writes_a_supersampled_still(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "still.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "40x37"
    got = np.fromfile(out, dtype=np.float32)
    assert got.size == 40 * 37 * 4
    got = got.reshape(37, 40, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    assert np.array_equal(_bits(got), _bits(r2.render_still(samples=4))), "the C++ host's still differs from the Python host's"
    assert (got[..., 3] == 1.0).all() and np.isfinite(got).all()
