"""-m gpu: point stars in stills - the catalogue of set_stars lensed into every sample's image of the accumulation (bhray_accum_set_stars).

Every comparison is bit for bit against the restatement (tests/accum_stars_ref.py) over the device's OWN trace results for the rays of accum_sample_rays, so nothing
of it depends on how the rays were traced.

   1. The mean of 5 samples is the restatement in every word: three shapes, both integrators, the box; the coverage floors on the 40 x 36 window.
   2. Switch off with a catalogue, switch on without one: the bits of a ctx that never saw either call; turning the switch off again restores them.
   3. The grouping of samples into calls and launches changes no word.
   4. The pixels sample 0 changed are the pixels star_kernel changes over the levels = 1 frame of the same size (bhray_diag_star_image).
   5. Under a tent and the Mitchell cubic the mean is the filter restatement over the starred images.
   6. The equirect still: periodic in x on a whole-width window, plain borders on a narrower one.
   7. The fisheye of fov pi.
   8. A gain that saturates: the mean is finite and at most 65504, and the display read is post_ref of its binary16 rounding.
   9. A catalogue replaced between two accum_add calls.
  10. The refusals.
  11. Frames keep their bits.
  12. Renderer.render_still(stars=True) and bhray_render --spp --stars-seeded.

Frames: ladder_for_frame((40, 36), 3, 2), a window of its 40 x 37 last level; 33 x 32; and 70 x 35 - accum_star_kernel's block owns a 64 x 4 pixel tile, so 70 x 35 is
the smallest frame with two tile columns, a partial tile in x and a row count that is no multiple of 4."""
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from bhusie_amd.cameras import StillCamera
from bhusie_amd.renderer import StillFilter
from tests import accum_filter_ref as FR
from tests import accum_ref as A
from tests import accum_stars_ref as AS
from tests import common as T
from tests import post_ref as P
from tests import stars_ref as S

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
THIRD = 1.0 / 3.0
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1),
        "70x35_two_tile_columns": lambda: B.ladder_from_base((70, 35), 3, 1)}
WINDOW = "40x36_of_a_ladder"
FILTERS = {"tent_1.5": (StillFilter.tent(1.5), FR.tent(1.5)), "mitchell_2": (StillFilter.mitchell(2.0), FR.cubic(2.0, THIRD, THIRD))}
catalogue = S.catalogue


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(cfg=None, method=1, stars=None, params=None, on=None):
    cam, bh = S.scene("default")
    rp = B.RayPass(cfg if cfg is not None else CFGS[WINDOW](), device=0)
    rp.set_textures(*T.textures())
    rp.set_uniforms(*T.uniforms(camera=cam, black_hole=bh, integration_method=method))
    if stars is not None:
        rp.set_stars(stars, layouts.BhrayStarParams.default(**params) if params else None)
    if on is not None:
        rp.accum_set_stars(on)
    return rp


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _accumulate(rp, groups):
    rp.accum_begin()
    for g in groups:
        rp.accum_add(g)
    return rp.accum_read()


def _own_results(rp, n):
    """the device's trace results, as (h, w, 4) images, for the rays it generates itself for samples 0 .. n - 1 under the uniforms and the still camera in force; a
    record without a direction (a fisheye sample outside the circle) is left out of the call and entered as (0, 0, 0, -1)"""
    h, w = int(rp.cfg.frame_h), int(rp.cfg.frame_w)
    out = []
    for s in range(n):
        rec = rp.accum_sample_rays(s)
        usable = (rec[:, 4:7] != 0.0).any(axis=1)
        r = np.zeros((rec.shape[0], 4), np.float32)
        r[:, 3] = -1.0
        r[usable] = rp.trace_rays(np.ascontiguousarray(rec[usable]))
        out.append(r.reshape(h, w, 4))
    return out


_STARRED = {}


def _starred(image, cat, params=None, wrap=False):
    """accum_stars_ref.starred, computed once per (image, catalogue, params, wrap): the tests share the device's sample images, and the restatement is a Python loop"""
    key = (image.tobytes(), cat.tobytes(), tuple(sorted((params or {}).items())), bool(wrap))
    if key not in _STARRED:
        _STARRED[key] = AS.starred(image, cat, params, T.textures()[2], wrap)
    return _STARRED[key]


def _restated(per_sample, cat, params=None, wrap=False, filt=None):
    """(mean, [T_s], [add_s], [st_s]) of the restatement over the device's sample images"""
    parts = [_starred(r, cat, params, wrap) for r in per_sample]
    mean, _ = AS.mean([p[0] for p in parts], T.textures()[2], filt)
    return mean, [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]


def _assert_words(got, want, what):
    differ = int((_bits(got.reshape(-1, 4)) != _bits(want)).sum())
    print(f"{what}: {differ} of {want.size} words differ")
    assert differ == 0, f"{what}: {differ} of {want.size} words differ from the restatement over the device's results"


# ---- 1. the mean, to the bit ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_mean_is_the_restatement_over_the_devices_own_results(shape, method):
    n = 5
    rp = _ctx(CFGS[shape](), method)
    per = _own_results(rp, n)
    want, _, adds, sts = _restated(per, catalogue())
    plain = _accumulate(rp, [n])
    rp.set_stars(catalogue())
    rp.accum_set_stars(True)
    got = _accumulate(rp, [n])
    assert rp.accum_samples() == n and got.shape == (rp.cfg.frame_h, rp.cfg.frame_w, 4) and got.dtype == np.float32
    lit = [a[..., 3] > 0 for a in adds]
    changed = int((_bits(got) != _bits(plain)).any(axis=-1).sum())
    print(shape, method, [S.floors(st) for st in sts], "pixels of the mean changed:", changed)
    assert all(m.sum() >= 10 for m in lit) and changed >= 10
    if shape == WINDOW:
        for st in sts:
            fl = S.floors(st)
            assert fl["lit"] >= 40 and fl["reversed"] >= 10, fl
        assert int((lit[0] != lit[1]).sum()) >= 20, "the lit sets of samples 0 and 1"
        assert changed >= 100, "pixels of the mean that differ from the starless mean"
    _assert_words(got, want, f"{shape} method {method}")
    rp.close()


# ---- 2. off is off ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_switch_without_a_catalogue_and_a_catalogue_without_the_switch_keep_every_bit():
    never = _ctx()
    want = _accumulate(never, [3])
    never.close()
    rp = _ctx(stars=catalogue(), on=False)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want)), "a catalogue with the switch off"
    rp.close()
    rp = _ctx(on=True)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want)), "the switch on without a catalogue"
    rp.set_stars(catalogue())
    starred = _accumulate(rp, [3])
    assert not np.array_equal(_bits(starred), _bits(want))
    rp.accum_set_stars(False)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want)), "the switch turned off again"
    rp.accum_set_stars(True)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(starred))
    rp.set_stars(None)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want)), "the catalogue removed"
    rp.close()


# ---- 3. grouping --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [WINDOW, "70x35_two_tile_columns"])
def test_the_grouping_of_samples_changes_no_word(shape):
    rp = _ctx(CFGS[shape](), stars=catalogue(), on=True)
    npix = rp.cfg.frame_w * rp.cfg.frame_h
    whole = _accumulate(rp, [5])
    assert np.array_equal(_bits(_accumulate(rp, [2, 3])), _bits(whole)), "add(2); add(3) differs from add(5)"
    rp.accum_set_launch_rays(npix)                                # K = 1: five launches, the kernel's grid one sample deep
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole)), "one sample per launch differs from five in one"
    rp.accum_set_launch_rays(2 * npix + 7)                        # K = 2: launches of 2, 2, 1
    assert np.array_equal(_bits(_accumulate(rp, [5])), _bits(whole))
    rp.accum_set_launch_rays(0)
    assert rp.accum_samples() == 5
    rp.close()


# ---- 4. the frame path's lit set ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["33x32_one_level", "70x35_two_tile_columns"])
def test_sample_0_lights_the_pixels_star_kernel_lights(shape):
    """Sample 0 is the pixel centre: its rays are the levels = 1 frame's.  A lit pixel receives at least flux_min / max_footprint^2 = 3e-6 per channel - above half an
    ulp of its sky^4 <= 1 in binary32, and a binary16 number over the zero image star_image starts from - so "changed" is "accepted a star" on both paths."""
    rp = _ctx(CFGS[shape]())
    plain = _accumulate(rp, [1])
    rp.set_stars(catalogue())
    rp.accum_set_stars(True)
    got = _accumulate(rp, [1])
    changed = (_bits(got) != _bits(plain)).any(axis=-1)
    rp.render()
    frame = rp.read_hdr()
    by_kernel = (rp.star_image(frame).view(np.uint16) != 0).any(axis=-1)
    add = _starred(_own_results(rp, 1)[0], catalogue())[1]
    print(shape, int(changed.sum()), int(by_kernel.sum()))
    assert changed.sum() >= 10 and np.array_equal(changed, by_kernel) and np.array_equal(changed, add[..., 3] > 0)
    rp.close()


# ---- 5. filters -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("shape", [WINDOW, "70x35_two_tile_columns"])
def test_a_filter_is_the_stars_point_spread_function(shape, name):
    n = 5
    filt, ref = FILTERS[name]
    rp = _ctx(CFGS[shape](), stars=catalogue(), on=True)
    want, _, adds, _ = _restated(_own_results(rp, n), catalogue(), filt=ref)
    rp.accum_set_filter(filt)
    got = _accumulate(rp, [n])
    _assert_words(got, want, f"{shape} {name}")
    rp.accum_set_filter(None)
    box = _accumulate(rp, [n])
    lit = np.any([a[..., 3] > 0 for a in adds], axis=0)
    spread = (_bits(got) != _bits(box)).any(axis=-1) & ~lit
    assert spread.sum() >= 10, "a filter carries a star's light into pixels that no star lies in"
    rp.close()


# ---- 6. equirect ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_whole_width_equirect_still_is_periodic_in_x():
    rp = _ctx()
    assert rp.cfg.crop_x == 0 and rp.cfg.frame_w == rp.cfg.level_w[rp.cfg.levels - 1]
    rp.accum_set_camera(StillCamera.equirect())
    per = _own_results(rp, 2)
    want, _, adds, sts = _restated(per, catalogue(), wrap=True)
    rp.set_stars(catalogue())
    rp.accum_set_stars(True)
    got = _accumulate(rp, [2])
    w = int(rp.cfg.frame_w)
    seam = [int((a[:, [0, w - 1], 3] > 0).sum()) for a in adds]
    print("equirect:", [S.floors(st) for st in sts], "lit in the first and last column:", seam)
    assert all(v >= 5 for v in seam), seam
    _assert_words(got, want, "equirect, wrapped")
    unwrapped = _restated(per, catalogue(), wrap=False)[0]
    assert not np.array_equal(_bits(unwrapped), _bits(want))
    rp.close()


@pytest.mark.parametrize("frame", [(39, 35), (38, 36)], ids=["39_of_40_from_column_0", "38_of_40_from_column_1"])
def test_a_narrower_equirect_window_has_plain_borders(frame):
    cfg = B.ladder_for_frame(frame, 3, 2)
    assert cfg.frame_w < cfg.level_w[cfg.levels - 1] and cfg.crop_x == (0 if frame[0] == 39 else 1)
    rp = _ctx(cfg)
    rp.accum_set_camera(StillCamera.equirect())
    per = _own_results(rp, 2)
    want, _, adds, _ = _restated(per, catalogue(), wrap=False)
    assert all(not (a[:, [0, frame[0] - 1], 3] > 0).any() and (a[..., 3] > 0).sum() >= 100 for a in adds)
    rp.set_stars(catalogue())
    rp.accum_set_stars(True)
    _assert_words(_accumulate(rp, [2]), want, f"equirect window {frame}")
    rp.close()


# ---- 7. fisheye -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fisheye_of_fov_pi():
    rp = _ctx()
    rp.accum_set_camera(StillCamera.fisheye(3.14159274))
    per = _own_results(rp, 2)
    want, _, adds, _ = _restated(per, catalogue())
    rp.set_stars(catalogue())
    rp.accum_set_stars(True)
    got = _accumulate(rp, [2])
    outside = np.all([r[..., 3] == -1.0 for r in per], axis=0)
    print("fisheye lit:", [int((a[..., 3] > 0).sum()) for a in adds], "outside the circle:", int(outside.sum()))
    assert all((a[..., 3] > 0).sum() >= 300 for a in adds) and outside.sum() >= 400
    assert np.array_equal(got[outside], np.broadcast_to(np.float32([0, 0, 0, 1]), got[outside].shape)), "out-of-circle pixels are black with alpha 1"
    _assert_words(got, want, "fisheye")
    rp.close()


# ---- 8. saturation ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_saturating_gain_stops_at_65504():
    params = dict(gain=1e6)
    rp = _ctx()
    per = _own_results(rp, 4)
    want, Ts, _, _ = _restated(per, catalogue(), params)
    assert any((t[..., 0:3] == 65504.0).any() for t in Ts), "the gain must drive some pixel past 65504"
    rp.set_stars(catalogue(), layouts.BhrayStarParams.default(**params))
    rp.accum_set_stars(True)
    got = _accumulate(rp, [4])
    assert np.isfinite(got).all() and float(got.max()) <= 65504.0 and float(got.max()) >= 65504.0 / 4   # (a pixel saturates in some samples, not in all four)
    _assert_words(got, want, "gain 1e6")
    disp = rp.accum_read_display()
    assert np.array_equal(disp, P.post_ref(got.astype(np.float16))), "the display read differs from post_ref over the binary16 mean"
    rp.close()


# ---- 9. the catalogue replaced ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_catalogue_replaced_between_two_adds_waits_for_the_first():
    cat_a, cat_b = catalogue(), assets.star_catalogue(2000, S.SEED + 1)
    rp = _ctx()
    per = _own_results(rp, 5)
    tex = T.textures()[2]
    want = AS.mean([_starred(r, cat_a if s < 3 else cat_b)[0] for s, r in enumerate(per)], tex)[0]
    rp.set_stars(cat_a)
    rp.accum_set_stars(True)
    rp.accum_begin()
    rp.accum_add(3)
    rp.set_stars(cat_b)                                           # at once: frees the buffers the outstanding samples read, behind a wait for them
    rp.accum_add(2)
    got = rp.accum_read()
    _assert_words(got, want, "catalogue A for samples 0 - 2, B for 3 and 4")
    assert not np.array_equal(_bits(got.reshape(-1, 4)), _bits(_restated(per, cat_a)[0]))
    rp.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals():
    rp = _ctx(stars=catalogue(), on=True)
    assert B.lib().bhray_accum_set_stars(rp._h, 2) == E_INVALID and B.lib().bhray_accum_set_stars(rp._h, -1) == E_INVALID
    rp.accum_begin()
    rp.accum_add(2)                                               # (the refused setter left the switch on)
    image = rp.accum_read()
    starless = _ctx()
    assert not np.array_equal(_bits(image), _bits(_accumulate(starless, [2])))
    starless.close()
    rp.accum_set_camera(StillCamera.pinhole(0.05, 19.0))          # accepted: the refusal belongs to accum_add
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    assert rp.accum_samples() == 2 and np.array_equal(_bits(rp.accum_read()), _bits(image))
    rp.accum_begin()
    assert _code(lambda: rp.accum_add_adaptive(2, 6, 2)) == E_STATE, "a lens and the stars"
    rp.accum_set_camera(None)
    assert _code(lambda: rp.accum_add_adaptive(2, 6, 2)) == E_STATE, "the stars alone"
    assert rp.accum_samples() == 0 and not rp.accum_read().any()
    rp.accum_set_stars(False)
    rp.accum_add_adaptive(2, 6, 2)                                # the switch off: adaptive stills as before, a lens as before
    rp.accum_set_camera(StillCamera.pinhole(0.05, 19.0))
    _accumulate(rp, [2])
    rp.accum_set_stars(True)
    rp.set_stars(None)
    _accumulate(rp, [2])                                          # the switch on without a catalogue refuses nothing
    rp.accum_begin()
    rp.accum_add_adaptive(2, 6, 2)
    rp.close()


# ---- 11. frames -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_frames_keep_their_bits_across_a_starred_still():
    rp = _ctx(stars=catalogue())

    def frame():
        rp.render()
        rp.resolve_display()
        return rp.read_hdr().copy(), rp.read_sky().copy(), rp.read_display().copy()
    before = frame()
    rp.accum_set_stars(True)
    again = frame()
    _accumulate(rp, [3])
    held = rp.read_hdr().copy(), rp.read_sky().copy(), rp.read_display().copy()
    after = frame()
    for a in (again, held, after):
        assert np.array_equal(_bits(a[0]), _bits(before[0])) and np.array_equal(a[1].view(np.uint16), before[1].view(np.uint16)) and np.array_equal(a[2], before[2])
    rp.close()


# ---- 12. hosts ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_render_still_takes_the_stars():
    r = B.Renderer(CFGS[WINDOW](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    r.set_stars(catalogue())
    still = r.render_still(samples=4, stars=True)
    want = _restated(_own_results(r.ray_pass, 4), catalogue())[0]
    _assert_words(still, want, "Renderer.render_still(stars=True)")
    plain = r.render_still(samples=4)                             # stars=False: the switch is off again
    rp = _ctx()
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    assert np.array_equal(_bits(plain), _bits(_accumulate(rp, [4]))) and not np.array_equal(_bits(plain), _bits(still))
    rp.close()
    with pytest.raises(ValueError):
        r.render_still(adaptive=B.AdaptiveStill(2, 6, 2), stars=True)
    r.render_still(samples=2, stars=True)
    r.render_still(adaptive=B.AdaptiveStill(2, 6, 2))             # an adaptive still after a starred one: the switch is put back
    r.ray_pass.close()


def test_cpp_host_writes_a_starred_still(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "still.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp", "4", "--stars-seeded", "2000", str(S.SEED)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "40x37"
    got = np.fromfile(out, dtype=np.float32).reshape(37, 40, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    plain = r2.render_still(samples=4)
    per = _own_results(r2.ray_pass, 4)
    parts = [AS.starred(p, catalogue(), None, grey) for p in per]
    assert all((p[1][..., 3] > 0).sum() >= 20 for p in parts)
    want = AS.mean([p[0] for p in parts], grey)[0]
    _assert_words(got, want, "bhray_render --spp 4 --stars-seeded 2000 1")
    assert not np.array_equal(_bits(got), _bits(plain))
    r2.ray_pass.close()
