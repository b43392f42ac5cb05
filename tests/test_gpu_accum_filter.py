"""-m gpu: still pixel filters - tent and cubic reconstruction of the accumulation image (bhray_accum_set_filter).

  1. The mean is, in every word, the restatement (tests/accum_filter_ref.py) over the device's own trace results for the rays of accum_sample_rays.
  2. The grouping of samples into calls and launches changes no word; begin clears.
  3. One sample under a filter that weighs (0, 0, 1, 0, 0) at s = 0 is the box's, bit for bit; set_filter(None) leaves a box accumulation as on a ctx that never
     saw the call.
  4. Samples that are not finite are skipped under the taps of their neighbours too: the mean is finite and the restatement's.
  5. A fisheye still and a thin-lens still under the Mitchell filter.
  6. The display read is tests/post_ref.py over the binary16 mean, byte for byte.
  7. The refusals.
  8. Renderer.render_still / save_still (filter=...) and bhray_render --filter.
  9. The mean against the restatement fed with the oracle's trace_ray of every sample.

Frames: tests/test_gpu_accum.py's two - ladder_for_frame((40, 36), 3, 2), a window of its 40 x 37 last level, and 33 x 32 -; a 5 x 3 single-level frame, smaller than
the filter's 5 x 5 support; and 70 x 19: accum_filter_add_kernel's block owns a 32 x 8 pixel tile (a 36 x 12 LDS copy with the halo of 2), so 70 x 19 is two whole
tiles and a partial one of 6 columns across, two whole tiles and a partial one of 3 rows down."""
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from bhusie_amd.cameras import StillCamera
from bhusie_amd.renderer import StillFilter
from tests import accum_filter_ref as FR
from tests import accum_ref as A
from tests import common as T
from tests import post_ref as P
from tests.test_gpu_accum import CAM, FAR, HOLE_AWAY_NAN, _oracle_samples

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
THIRD = 1.0 / 3.0
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1),
        "5x3_below_the_support": lambda: B.ladder_from_base((5, 3), 3, 1), "70x19_three_tiles_each_way": lambda: B.ladder_from_base((70, 19), 3, 1)}
FILTERS = {"tent_1.5": (StillFilter.tent(1.5), FR.tent(1.5)), "mitchell_2": (StillFilter.mitchell(2.0), FR.cubic(2.0, THIRD, THIRD))}
MITCHELL = FILTERS["mitchell_2"]
UNIT_AT_0 = {"tent_1": StillFilter.tent(1.0), "catmull_rom_2": StillFilter(B.layouts.FILTER_CUBIC, 2.0, 0.0, 0.5)}
NEAR = B.Camera(position=(0.0, 1.5, -6.0), forward=(0.0, -0.25, 1.0), fov=1.3)         # tests/test_gpu_still_camera.py's scenes
LENS_CAM = B.Camera(position=(0.0, 2.0, -12.0), forward=(0.0, -0.16, 1.0), fov=1.3)


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


def _wh(cfg):
    return int(cfg.frame_w), int(cfg.frame_h)


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


def _own_results(rp, S):
    """the device's trace results for the rays it generates itself for samples 0 .. S - 1 under the uniforms and the still camera in force"""
    return [_trace(rp, rp.accum_sample_rays(s)) for s in range(S)]


def _restated(rp, ref, per_sample):
    w, h = _wh(rp.cfg)
    total = FR.accumulate(per_sample, T.textures()[2], ref, w, h)
    return A.mean(total), total


def _assert_words(got, want, what):
    differ = int((_bits(got.reshape(-1, 4)) != _bits(want)).sum())
    print(f"{what}: {differ} of {want.size} words differ")
    assert differ == 0, f"{what}: {differ} of {want.size} words differ from the restatement over the device's results"


# ---- 1. the mean, to the bit --------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_mean_is_the_restatement_over_the_devices_own_results(shape, name, method):
    S = 5
    filt, ref = FILTERS[name]
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method))
    want, total = _restated(rp, ref, _own_results(rp, S))
    rp.accum_set_filter(filt)
    got = _accumulate(rp, [S])
    assert rp.accum_samples() == S and got.shape == (rp.cfg.frame_h, rp.cfg.frame_w, 4) and got.dtype == np.float32
    assert (total[:, 3] > 0).all() and (got[..., 3] == 1.0).all()
    if name == "mitchell_2" and shape != "5x3_below_the_support":
        w, h = _wh(rp.cfg)
        weight = total[:, 3].reshape(h, w)
        assert weight[0, 0] < weight[h // 2, 0] < weight[h // 2, w // 2], "border pixels receive less weight and renormalise by themselves"
    _assert_words(got, want, f"{shape} {name} method {method}")


# ---- 2. grouping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", ["40x36_of_a_ladder", "70x19_three_tiles_each_way"])
def test_the_grouping_of_samples_changes_no_word(shape, method):
    rp = _ctx(CFGS[shape]())
    npix = rp.cfg.frame_w * rp.cfg.frame_h
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method))
    rp.accum_set_filter(MITCHELL[0])
    whole = _accumulate(rp, [5])
    assert np.array_equal(_bits(_accumulate(rp, [2, 3])), _bits(whole)), "add(2); add(3) differs from add(5)"
    rp.accum_set_launch_rays(npix)                                # K = 1: five launches
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole)), "one sample per launch differs from five in one"
    rp.accum_set_launch_rays(2 * npix + 7)                        # K = 2: launches of 2, 2, 1
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole))
    rp.accum_set_launch_rays(0)
    assert rp.accum_samples() == 5
    rp.accum_begin()                                              # clears
    assert rp.accum_samples() == 0 and not rp.accum_read().any()
    assert not np.array_equal(_bits(_accumulate(rp, [4])), _bits(whole))
    rp.accum_set_filter(None)
    assert not np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole)), "the filter must change the image"


# ---- 3. the box -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_one_centre_sample_is_the_boxs_and_null_restores_the_box(method):
    u = T.uniforms(camera=CAM, integration_method=method)
    never = _ctx()
    never.set_uniforms(*u)
    box1, box5 = _accumulate(never, [1]), _accumulate(never, [5])
    rp = _ctx()
    rp.set_uniforms(*u)
    for name, filt in UNIT_AT_0.items():
        assert [list(w) for w in filt.weights(0)] == [[0, 0, 1, 0, 0]] * 2
        rp.accum_set_filter(filt)
        assert np.array_equal(_bits(_accumulate(rp, [1])), _bits(box1)), f"{name}: one sample differs from the box's"
        assert not np.array_equal(_bits(_accumulate(rp, [5])), _bits(box5))
    rp.accum_set_filter(None)
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(box5)), "after set_filter(None) the box accumulation differs from a ctx that never saw the call"
    rp.accum_set_filter(StillFilter())                           # the explicit box struct
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(box5))


# ---- 4. skipped samples ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_samples_that_are_not_finite_are_skipped_under_every_tap(name, method):
    S = 5
    filt, ref = FILTERS[name]
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=FAR, black_hole=HOLE_AWAY_NAN, integration_method=method))
    per_sample = _own_results(rp, S)
    w, h = _wh(rp.cfg)
    touched = FR.skipped_in_support(per_sample, T.textures()[2], ref, w, h)
    print(f"{name} method {method}: {int(touched.sum())} pixels have a skipped sample under a tap of non-zero weight")
    assert int(touched.sum()) >= 20
    want, total = _restated(rp, ref, per_sample)
    rp.accum_set_filter(filt)
    got = _accumulate(rp, [S])
    assert np.isfinite(got).all(), "a sample that is not finite reached a mean"
    _assert_words(got, want, f"hole away, {name} method {method}")


# ---- 5. still cameras ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("kind", ["fisheye", "lens"])
def test_a_still_camera_under_the_mitchell_filter(kind, method):
    S = 4
    still, cam = {"fisheye": (StillCamera.fisheye(3.4), NEAR), "lens": (StillCamera.pinhole(lens_radius=0.3, focus_distance=12.0), LENS_CAM)}[kind]
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=method))
    rp.accum_set_camera(still)
    per_sample = _own_results(rp, S)
    if kind == "fisheye":
        outside = np.stack([r[:, 3] == -1.0 for r in per_sample])
        assert outside.all(axis=0).any() and not outside.all(), "the out-of-circle (0, 0, 0, -1) is a finite black sample and takes part"
    want, total = _restated(rp, MITCHELL[1], per_sample)
    rp.accum_set_filter(MITCHELL[0])
    got = _accumulate(rp, [S])
    _assert_words(got, want, f"{kind} method {method}")


# ---- 6. display ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILTERS))
def test_the_display_read_is_post_ref_of_the_rounded_mean(name):
    rp = _ctx(CFGS["33x32_one_level"]())
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=1))
    rp.accum_set_filter(FILTERS[name][0])
    mean = _accumulate(rp, [4])
    disp = rp.accum_read_display()
    assert disp.shape == (32, 33, 4) and disp.dtype == np.uint8
    with np.errstate(over="ignore"):
        sky16 = mean.astype(np.float16)                           # nearest even
    assert np.array_equal(disp, P.post_ref(sky16)), "the display read differs from post_ref over the binary16 mean"
    assert np.array_equal(_bits(rp.accum_read()), _bits(mean)), "the display read changed the mean"


# ---- 7. refusals --------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    u = T.uniforms(camera=CAM, integration_method=1)
    adaptive = {"min_samples": 2, "max_samples": 6, "round_samples": 2, "tolerance": 0.05, "dark": 0.01}
    rp = _ctx()
    rp.accum_set_filter(MITCHELL[0])                              # accepted before begin and before the uniforms
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    rp.accum_begin()
    assert _code(lambda: rp.accum_add(1)) == E_STATE              # before the first set_uniforms
    rp.set_uniforms(*u)
    # add_adaptive under a filter is refused with nothing enqueued, and works under the box afterwards
    assert _code(lambda: rp.accum_add_adaptive(**adaptive)) == E_STATE
    assert rp.accum_samples() == 0 and not rp.accum_read().any()
    rp.accum_set_filter(None)
    rp.accum_begin()
    info = rp.accum_add_adaptive(**adaptive)
    plain = _ctx()
    plain.set_uniforms(*u)
    plain.accum_begin()
    assert plain.accum_add_adaptive(**adaptive) == info
    adaptive_mean = rp.accum_read()
    assert np.array_equal(_bits(adaptive_mean), _bits(plain.accum_read()))
    # add under a filter after an adaptive call stays refused
    rp.accum_set_filter(MITCHELL[0])
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    assert np.array_equal(_bits(rp.accum_read()), _bits(adaptive_mean))
    # an invalid struct leaves the filter in force untouched
    rp.accum_set_filter(FILTERS["tent_1.5"][0])
    tent = _accumulate(rp, [3])
    L, h = rp._L, rp._h

    def bad(**kw):
        s = MITCHELL[0].struct()
        for k, v in kw.items():
            setattr(s, k, v)
        rc = L.bhray_accum_set_filter(h, C.byref(s))
        if rc != 0:
            assert L.bhray_last_error(h), "a refusal carries a message"
        return rc
    nan = float("nan")
    for kw in ({"struct_size": 16}, {"kind": 3}, {"radius": 0.9}, {"radius": 2.6}, {"radius": nan}, {"b": 1.5}, {"c": -0.5}, {"c": nan}, {"kind": 1, "radius": 0.4}):
        assert bad(**kw) == E_INVALID, kw
    assert _code(lambda: rp.accum_set_filter(StillFilter.tent(3.0))) == E_INVALID
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(tent)), "a refused filter changed the filter in force"
    assert bad() == 0
    assert not np.array_equal(_bits(_accumulate(rp, [3])), _bits(tent))
    # every refusal of bhray_accum_add stays on bhray_accum_add
    rp.accum_begin()
    rp.set_mesh_lensing(True)
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    rp.set_mesh_lensing(False)
    rp.accum_add(1)
    assert _code(lambda: rp.accum_add(65536)) == E_INVALID
    for kw in ({"literal": True}, {"eval_fma": True}, {"devices": [0, 0]}, {"row_rank": 0, "row_world": 2}):
        q = _ctx(**kw)
        q.set_uniforms(*u)
        q.accum_set_filter(MITCHELL[0])                           # validates and stores (a multi-device ctx forwards it): accepted
        assert _code(lambda: q.accum_set_filter(StillFilter.tent(0.1))) == E_INVALID, kw
        assert _code(q.accum_begin) == E_STATE, kw
        assert _code(lambda: q.accum_add(1)) == E_STATE, kw


def test_frames_keep_their_bits_across_a_filter_change():
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=1))
    rp.render()
    frame = rp.read_hdr().copy()
    rp.accum_set_filter(MITCHELL[0])
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed with the still filter"
    _accumulate(rp, [3])
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed behind a filtered still"


# ---- 8. hosts -----------------------------------------------------------------------------------------
def test_render_still_and_save_still_take_the_filter(tmp_path):
    r = B.Renderer(CFGS["40x36_of_a_ladder"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    still = r.render_still(samples=4, filter=StillFilter.mitchell())
    rp = _ctx()
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    rp.accum_set_filter(StillFilter.mitchell())
    assert np.array_equal(_bits(still), _bits(_accumulate(rp, [4]))), "render_still(filter=...) differs from the RayPass sequence"
    plain = r.render_still(samples=4)                             # filter=None: the box again
    rp.accum_set_filter(None)
    assert np.array_equal(_bits(plain), _bits(_accumulate(rp, [4]))) and not np.array_equal(_bits(plain), _bits(still))
    with pytest.raises(ValueError):
        r.render_still(adaptive=B.AdaptiveStill(2, 6, 2), filter=StillFilter.tent())
    r.render_still(samples=2, filter=StillFilter.tent())
    r.render_still(adaptive=B.AdaptiveStill(2, 6, 2))             # an adaptive still after a filtered one: the box is put back
    from PIL import Image
    path = tmp_path / "still.png"
    r.save_still(path, samples=4, filter=StillFilter.bspline())
    rp.accum_set_filter(StillFilter.bspline())
    _accumulate(rp, [4])
    want8 = rp.accum_read_display()
    want8[..., 3] = 255
    assert np.array_equal(np.asarray(Image.open(path).convert("RGBA")), want8)


def test_cpp_host_writes_a_filtered_still(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "still.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp", "4", "--filter", "cubic", "2", "0.3333333", "0.3333333"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "40x37"
    got = np.fromfile(out, dtype=np.float32).reshape(37, 40, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    want = r2.render_still(samples=4, filter=StillFilter(B.layouts.FILTER_CUBIC, 2.0, 0.3333333, 0.3333333))
    assert np.array_equal(_bits(got), _bits(want)), "the C++ host's still differs from the Python host's"
    assert not np.array_equal(_bits(got), _bits(r2.render_still(samples=4)))


# ---- 9. oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_the_mean_against_the_oracle(name, method):
    """tests/test_gpu_accum.py's test 4 - its scene, frame, rays and oracle samples (shared: computed once) - under a filter: the restatement fed with the oracle's
    trace_ray results against the device mean.  Every sample's colour is within REL_TOL of max(|want|, floor), so a mean with non-negative weights is within
    2 REL_TOL max(mean, floor); each pixel's sum is N = 25 S additions (a product before each) and a division, one rounding each; negative lobes amplify both by
    kappa = max over pixels of sum |w| / |sum w| (1 for the tent).  Measured on an MI355X, S = 4: tent 1.5 max relative error 2.1e-7 (euler) and 2.4e-7
    (rk) at a bar of 2.12e-4; Mitchell 2, kappa 1.139: 1.9e-6 and 9.3e-7 at a bar of 2.41e-4."""
    S = 4
    filt, ref = FILTERS[name]
    per_sample = _oracle_samples(method, S)
    cfg = CFGS["40x36_of_a_ladder"]()
    w, h = _wh(cfg)
    tex = T.textures()[2]
    want = A.mean(FR.accumulate(per_sample, tex, ref, w, h))
    kappa = FR.kappa(per_sample, tex, ref, w, h)
    assert kappa == 1.0 if ref.kind == FR.TENT else 1.0 < kappa < 2.0
    rp = _ctx(cfg)
    rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method))
    rp.accum_set_filter(filt)
    got = _accumulate(rp, [S]).reshape(-1, 4)
    assert np.array_equal(got[:, 3], want[:, 3])
    N = 25 * S
    bar = (2 * T.REL_TOL + (N + 1) * 2.0 ** -23) * kappa
    err = float(T.rel_err(got[:, 0:3], want[:, 0:3]).max())
    print(f"{name} method {method}: max rel err {err:.3g} (bar {bar:.3g}, kappa {kappa:.6g}), "
          f"bit-identical {100.0 * float((_bits(got) == _bits(want)).all(axis=1).mean()):.2f} %")
    assert err <= bar, f"max rel err {err:.3g} > {bar:.3g}"
