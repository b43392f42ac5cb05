"""-m gpu: still passes - coverage, geometry, position and escape maps per pixel beside a still's colour (bhray_accum_set_passes).

  1. Box filter: each pass is, in every word, the NumPy restatement (tests/accum_passes_ref.py) over the device's own results and records for the rays it generates.
  2. The grouping of samples into calls and launches changes no word; begin clears the planes.
  3. The colour keeps its bits with passes on; frames before and after keep theirs; with the set 0 there is no pass to read.
  4. One sample: COVERAGE is the one-hot of render_records' kind, GEOMETRY and POSITION are its record words.
  5. Tent and Mitchell: each pass is accum_filter_ref's stencil over the restated sample images in every word, border pixels included.
  6. Fisheye (pixels outside the circle: zero vectors, w = S), equirect and lens stills against the restatement.
  7. Point stars leave every pass its bits (the pass work runs before the star kernel); under an observer the passes are the restatement over the boosted rays.
  8. Skipped samples: w < S exactly where the restatement says, every mean finite.
  9. Refusals, and the running accumulation keeps its set.
 10. Renderer.render_still(passes=...) / still_pass and bhray_render --spp N --passes.
 11. Cost: a 1920 x 1080 still of 4 samples with the set 0 and with BHRAY_PASS_ALL, printed (no bar).

The scene is a mesh scene under set_mesh_lensing(LENS_FRAMES | LENS_RAYS) whose mesh straddles the relativity sphere, seen from just outside it, so that horizon,
disk, mesh and none are each the first hit of at least 16 pixels at sample 0 and pixels on their outlines have fractional coverage at S = 5 - asserted below from the
restatement over the device's records, never from the pass images.  The frames are tests/test_gpu_accum.py's."""
import os
import subprocess
import time

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from bhusie_amd.cameras import StillCamera
from bhusie_amd.layouts import HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH, HIT_UNUSABLE, PASS_COVERAGE, PASS_GEOMETRY, PASS_POSITION, PASS_ESCAPE, PASS_ALL
from bhusie_amd.renderer import StillFilter
from tests import accum_filter_ref as FR
from tests import accum_passes_ref as PR
from tests import common as T
from tests import rays_ref as RR
from tests import stars_ref as SR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
THIRD = 1.0 / 3.0
S5 = 5
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1)}
FILTERS = {"tent_1.5": (StillFilter.tent(1.5), FR.tent(1.5)), "mitchell_2": (StillFilter.mitchell(2.0), FR.cubic(2.0, THIRD, THIRD))}
PASSES = {"coverage": PASS_COVERAGE, "geometry": PASS_GEOMETRY, "position": PASS_POSITION, "escape": PASS_ESCAPE}
# from tests/test_gpu_accum.py's MESH_CAM / MESH_AT, moved in until the horizon fills 16 pixels of the 33 x 32 frame and the mesh reaches into the sphere (chosen on
# the CPU with tests/lensed_rays_ref.py's records of sample 0: horizon / disk / mesh / none = 20 / 90 / 66 / 880 of 1 056 pixels under RK, 27 / 87 / 59 / 883 under Euler)
PASS_CAM = B.Camera(position=(0.0, 2.5, -24.0), forward=(-0.15, -0.09, 1.0), fov=1.0)
PASS_AT = (-13.0, 5.0, -12.0)
LENSING = 3                                                       # LENS_FRAMES | LENS_RAYS
FAR = B.Camera(position=(2.0, 1.0, -45.0), forward=(0.0, 0.0, 1.0), fov=0.9)          # tests/test_gpu_accum.py's scene with samples that are not finite
HOLE_AWAY_NAN = B.BlackHole(position=(1.5, -0.75, 2.0))
NEAR = B.Camera(position=(0.0, 1.5, -6.0), forward=(0.0, -0.25, 1.0), fov=1.3)         # tests/test_gpu_still_camera.py's scenes
LENS_CAM = B.Camera(position=(0.0, 2.0, -12.0), forward=(0.0, -0.16, 1.0), fov=1.3)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _wh(cfg):
    return int(cfg.frame_w), int(cfg.frame_h)


def _ctx(cfg=None, method=1, camera=PASS_CAM, mesh=True, black_hole=None, **kw):
    rp = B.RayPass(cfg if cfg is not None else CFGS["40x36_of_a_ladder"](), device=0, **kw)
    rp.set_textures(*T.textures())
    if mesh:
        rp.upload_model(RR.mesh_model(PASS_AT))
    rp.set_uniforms(*T.uniforms(camera=camera, black_hole=black_hole, integration_method=method, model_count=1 if mesh else 0))
    if mesh:
        rp.set_mesh_lensing(LENSING)
    return rp


def _trace(rp, rays):
    """the device's results and records for one sample's generated rays; a record without a direction (a fisheye sample outside the circle) is left out of the call
    and entered as the device form answers it: (0, 0, 0, -1), hit = HIT_UNUSABLE, triangle = -1, every other word zero"""
    usable = (rays[:, 4:7] != 0.0).any(axis=1)
    res = np.zeros((rays.shape[0], 4), np.float32)
    res[:, 3] = -1.0
    rec = np.zeros(rays.shape[0], B.RAY_RECORD_DTYPE)
    rec["hit"] = HIT_UNUSABLE
    rec["triangle"] = -1
    if usable.any():
        res[usable], rec[usable] = rp.trace_rays_records(np.ascontiguousarray(rays[usable]))
    return res, rec


def _samples(rp, S):
    """(results, records, rays) of samples 0 .. S - 1 under the uniforms, the still camera and the observer in force"""
    out = []
    for s in range(S):
        rays = rp.accum_sample_rays(s)
        out.append(_trace(rp, rays) + (rays,))
    return out


def _want(rp, per_sample, filt=None):
    w, h = _wh(rp.cfg)
    return {name: PR.mean(PR.accumulate(per_sample, bit, filt, w, h)) for name, bit in PASSES.items()}


def _still(rp, groups, passes=PASS_ALL):
    rp.accum_set_passes(passes)
    rp.accum_begin()
    for g in groups:
        rp.accum_add(g)
    return {name: rp.accum_read_pass(bit).reshape(-1, 4) for name, bit in PASSES.items() if passes & bit}


def _assert_words(got, want, what):
    for name in want:
        differ = _bits(got[name]) != _bits(want[name])
        n = int(differ.sum())
        print(f"{what}, {name}: {n} of {differ.size} words differ")
        if n:
            p, ch = np.argwhere(differ)[0]
            raise AssertionError(f"{what}, {name}: {n} of {differ.size} words differ from the restatement; the first at pixel {p} channel {ch}: "
                                 f"{got[name][p, ch]!r} != {want[name][p, ch]!r}")


def _assert_scene(per_sample, what):
    """the scene holds what the tests are about - from the restatement over the records"""
    kind = PR.kinds(per_sample[0][1])
    counts = {k: int((kind == k).sum()) for k in (HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH)}
    cov = PR.mean(PR.accumulate(per_sample, PR.COVERAGE))
    fractional = int(((cov[:, 0:3] > 0) & (cov[:, 0:3] < 1)).any(axis=1).sum())
    print(f"{what}: first hits at sample 0 none / horizon / disk / mesh = {counts[HIT_NONE]} / {counts[HIT_HORIZON]} / {counts[HIT_DISK]} / {counts[HIT_MESH]}, "
          f"{fractional} pixels with a fractional coverage at S = {len(per_sample)}")
    assert min(counts.values()) >= 16, f"{what}: every kind must be the first hit of at least 16 pixels at sample 0: {counts}"
    assert fractional >= 4, f"{what}: {fractional} pixels with a fractional coverage"


# ---- 1. the restatement, box filter --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_every_pass_is_the_restatement_over_the_devices_own_records(shape, method):
    rp = _ctx(CFGS[shape](), method)
    per_sample = _samples(rp, S5)
    _assert_scene(per_sample, f"{shape} method {method}")
    got = _still(rp, [S5])
    assert rp.accum_passes() == PASS_ALL and rp.accum_samples() == S5
    w, h = _wh(rp.cfg)
    full = rp.accum_read_pass(PASS_COVERAGE)
    assert full.shape == (h, w, 4) and full.dtype == np.float32 and (full[..., 3] == 1.0).all()
    _assert_words(got, _want(rp, per_sample), f"{shape} method {method}")
    esc = got["escape"]
    length = np.sqrt((esc[:, 0:3].astype(np.float64) ** 2).sum(axis=1))
    assert (length <= 1.0 + 1e-5).all(), "an escape vector is a mean of unit directions and zeros"
    rp.close()


# ---- 2. grouping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_grouping_of_samples_changes_no_word(method):
    rp = _ctx(method=method)
    npix = int(np.prod(_wh(rp.cfg)))
    whole = _still(rp, [S5])
    _assert_words(_still(rp, [2, 3]), whole, "add(2); add(3)")
    rp.accum_set_launch_rays(npix)                                # one sample per launch
    _assert_words(_still(rp, [S5]), whole, "one sample per launch")
    rp.accum_set_launch_rays(2 * npix + 7)                        # launches of 2, 2, 1
    _assert_words(_still(rp, [S5]), whole, "launches of 2, 2, 1")
    rp.accum_set_launch_rays(0)
    rp.accum_begin()                                              # clears the planes
    for bit in PASSES.values():
        assert not rp.accum_read_pass(bit).any(), "begin leaves empty planes: w = 0 everywhere, so zeros"
    fewer = _still(rp, [4])
    assert any(not np.array_equal(_bits(fewer[n]), _bits(whole[n])) for n in whole)
    rp.close()


# ---- 3. the colour keeps its bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "mitchell_2"], ids=["box", "mitchell_2"])
def test_the_colour_and_the_frames_keep_their_bits(filt):
    rp = _ctx()
    rp.accum_set_filter(FILTERS[filt][0] if filt else None)
    rp.render()
    frame = rp.read_hdr().copy()
    rp.accum_set_passes(0)
    rp.accum_begin(); rp.accum_add(S5)
    plain = rp.accum_read()
    assert rp.accum_passes() == 0
    for bit in PASSES.values():
        assert _code(lambda: rp.accum_read_pass(bit)) == E_INVALID, "with the set 0 there is no pass to read"
    _still(rp, [S5])
    assert np.array_equal(_bits(rp.accum_read()), _bits(plain)), "the colour changed with BHRAY_PASS_ALL"
    one = _still(rp, [S5], PASS_GEOMETRY)
    assert np.array_equal(_bits(rp.accum_read()), _bits(plain)), "the colour changed with one pass"
    assert list(one) == ["geometry"] and _code(lambda: rp.accum_read_pass(PASS_COVERAGE)) == E_INVALID
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed with a still's passes beside it"
    rp.close()


# ---- 4. one sample -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_one_sample_is_the_record_of_the_pixel(method):
    cfg = CFGS["40x36_of_a_ladder"]()
    r = B.Renderer(cfg, device=0)
    r.ray_pass.set_textures(*T.textures())
    r.add_model(RR.mesh_model(PASS_AT))
    r.camera = PASS_CAM
    r.ray_details.integration_method = method
    r.mesh_lensing = True
    r.lens_ray_batches = True
    r.render_still(samples=1, passes=PASS_ALL)
    w, h = _wh(cfg)
    rec = r.render_records(r.ray_pass.accum_sample_rays(0), (h, w))
    kind = rec["hit"] & 0xFF
    assert all(int((kind == k).sum()) >= 16 for k in (HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH))
    cov, geo, pos = r.still_pass("coverage"), r.still_pass("geometry"), r.still_pass(PASS_POSITION)
    assert (cov[..., 3] == 1.0).all(), "the scene has no sample that is not finite"
    for ch, k in enumerate((HIT_HORIZON, HIT_DISK, HIT_MESH)):
        assert np.array_equal(cov[..., ch], (kind == k).astype(np.float32)), f"coverage channel {ch} is not the one-hot of the record's kind"
    assert np.array_equal(_bits(geo[..., 0]), _bits(rec["closest"])) and np.array_equal(_bits(geo[..., 2]), _bits(rec["transmittance"]))
    assert np.array_equal(geo[..., 1], rec["iterations"].astype(np.float32))
    solid = (kind == HIT_DISK) | (kind == HIT_MESH)
    assert np.array_equal(_bits(pos[..., 0:3][solid]), _bits(rec["position"][solid])) and not pos[..., 0:3][~solid].any()


# ---- 5. filters ----------------------------------------------------------------------------------------------------------------
# (RK on both frames; Euler on the single-level frame: the stencil does not depend on the integrator)
@pytest.mark.parametrize("shape, method", [("40x36_of_a_ladder", 1), ("33x32_one_level", 1), ("33x32_one_level", 0)], ids=["40x36_rk", "33x32_rk", "33x32_euler"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_a_filtered_pass_is_the_stencil_over_the_restated_sample_images(shape, name, method):
    rp = _ctx(CFGS[shape](), method)
    rp.accum_set_filter(FILTERS[name][0])
    per_sample = _samples(rp, S5)
    got = _still(rp, [S5])
    want = _want(rp, per_sample, FILTERS[name][1])
    _assert_words(got, want, f"{shape} {name} method {method}")
    w, h = _wh(rp.cfg)
    border = np.zeros((h, w), bool)
    border[:2] = border[-2:] = True; border[:, :2] = border[:, -2:] = True
    assert want["coverage"].reshape(h, w, 4)[border].any(), "the border pixels are part of the comparison"
    _assert_words(_still(rp, [2, 3]), want, f"{shape} {name} method {method}, added as 2 + 3")
    rp.close()


# ---- 6. cameras ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fisheye", "equirect", "lens"])
def test_a_still_camera(kind):
    still = {"fisheye": StillCamera.fisheye(3.4), "equirect": StillCamera.equirect(), "lens": StillCamera.pinhole(lens_radius=0.3, focus_distance=12.0)}[kind]
    rp = _ctx(CFGS["40x36_of_a_ladder"](), 1, camera=LENS_CAM if kind == "lens" else NEAR, mesh=False)
    rp.accum_set_camera(still)
    per_sample = _samples(rp, S5)
    got = _still(rp, [S5])
    _assert_words(got, _want(rp, per_sample), kind)
    if kind == "fisheye":                                         # 40 x 36: the circle (diameter 36) is smaller than the frame is wide
        outside = np.all([PR.kinds(q) == HIT_UNUSABLE for _, q, _ in per_sample], axis=0)
        assert int(outside.sum()) >= 40, "pixels wholly outside the image circle"
        for name, bit in PASSES.items():
            assert (PR.accumulate(per_sample, bit)[outside, 3] == S5).all(), "w = S outside the circle"
            assert not got[name][outside, 0:3].any() and (got[name][outside, 3] == 1.0).all(), f"{name}: a pixel outside the circle is a finite sample with a zero vector"
        assert not rp.accum_read().reshape(-1, 4)[outside, 0:3].any()
    rp.close()


# ---- 7. stars and observer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "tent_1.5"], ids=["box", "tent_1.5"])
def test_point_stars_leave_every_pass_its_bits(filt):
    rp = _ctx(mesh=False, camera=B.Camera())
    rp.accum_set_filter(FILTERS[filt][0] if filt else None)
    rp.set_stars(SR.catalogue())
    rp.accum_set_stars(False)
    off = _still(rp, [S5])
    plain = rp.accum_read()
    rp.accum_set_stars(True)
    on = _still(rp, [S5])
    assert not np.array_equal(_bits(rp.accum_read()), _bits(plain)), "the catalogue must be in the colour"
    _assert_words(on, off, f"stars on against stars off ({filt or 'box'})")
    assert on["escape"][:, 0:3].any()
    rp.close()


@pytest.mark.parametrize("beaming", [True, False], ids=["beaming", "aberration_only"])
def test_under_an_observer_the_passes_are_the_restatement_over_the_boosted_rays(beaming):
    rp = _ctx()
    at_rest = rp.accum_sample_rays(1)
    rp.accum_set_observer((0.3, -0.2, 0.4), beaming=beaming)
    per_sample = _samples(rp, S5)
    assert not np.array_equal(_bits(per_sample[1][2]), _bits(at_rest)), "the generated rays are the boosted ones"
    got = _still(rp, [S5])
    _assert_words(got, _want(rp, per_sample), f"observer, beaming {beaming}")
    rp.close()


# ---- 8. skipped samples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "mitchell_2"], ids=["box", "mitchell_2"])
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_samples_that_are_not_finite_are_skipped(method, filt):
    rp = _ctx(method=method, camera=FAR, mesh=False, black_hole=HOLE_AWAY_NAN)
    rp.accum_set_filter(FILTERS[filt][0] if filt else None)
    per_sample = _samples(rp, S5)
    n = np.sum([PR.taken(r) for r, _, _ in per_sample], axis=0)
    print(f"method {method}: samples taken per pixel {dict(zip(*np.unique(n, return_counts=True)))}")
    assert (n < S5).any(), "the scene must produce samples that are not finite"
    got = _still(rp, [S5])
    _assert_words(got, _want(rp, per_sample, FILTERS[filt][1] if filt else None), f"skipped samples, method {method}, {filt or 'box'}")
    assert all(np.isfinite(g).all() for g in got.values()), "a NaN sample reached a pass"
    if filt is None:
        rp.accum_set_passes(PASS_ALL); rp.accum_begin(); rp.accum_add(S5)
        for name, bit in PASSES.items():
            w = PR.accumulate(per_sample, bit)[:, 3]
            assert np.array_equal(w, n.astype(np.float32)), "the restatement's w is the number of samples taken"
            assert np.array_equal(got[name][:, 3] == 0.0, n == 0), f"{name}: alpha is 0 exactly where no sample was taken"
    rp.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_running_accumulation_keeps_its_set():
    rp = _ctx()
    assert rp.accum_passes() == 0
    assert _code(lambda: rp.accum_read_pass(PASS_COVERAGE)) == E_STATE          # before begin
    assert _code(lambda: rp.accum_set_passes(0x10)) == E_INVALID and _code(lambda: rp.accum_set_passes(0xFFFFFFFF)) == E_INVALID
    rp.accum_set_passes(PASS_COVERAGE | PASS_ESCAPE)
    assert rp.accum_passes() == 0, "in force from the next begin"
    assert _code(lambda: rp.accum_set_passes(PASS_ALL + 1)) == E_INVALID       # the stored set stays
    rp.accum_begin()
    assert rp.accum_passes() == PASS_COVERAGE | PASS_ESCAPE
    rp.accum_add(2)
    rp.accum_set_passes(PASS_GEOMETRY)                            # does not change the running accumulation
    assert rp.accum_passes() == PASS_COVERAGE | PASS_ESCAPE
    rp.accum_add(3)
    running = {n: rp.accum_read_pass(PASSES[n]).reshape(-1, 4) for n in ("coverage", "escape")}
    for bad in (PASS_GEOMETRY, PASS_POSITION, 0, PASS_COVERAGE | PASS_ESCAPE, 0x10, 0xFFFFFFFF):
        assert _code(lambda: rp.accum_read_pass(bad)) == E_INVALID, hex(bad)
    whole = _still(rp, [S5], PASS_COVERAGE | PASS_ESCAPE)
    _assert_words(running, whole, "2 + 3 with a set_passes between them")
    # adaptive stills carry no passes
    kw = dict(min_samples=2, max_samples=6, round_samples=2, tolerance=0.05, dark=0.01)
    rp.accum_set_passes(PASS_COVERAGE)
    rp.accum_begin()
    assert _code(lambda: rp.accum_add_adaptive(**kw)) == E_STATE
    assert rp.accum_samples() == 0, "a refused adaptive call enqueued something"
    rp.accum_add(1)                                               # the accumulation is still bhray_accum_add's to fill
    rp.accum_set_passes(0)
    rp.accum_begin()
    rp.accum_add_adaptive(**kw)
    assert rp.accum_passes() == 0
    # every existing refusal holds
    fresh = B.RayPass(CFGS["40x36_of_a_ladder"](), device=0)
    fresh.set_textures(*T.textures())
    fresh.accum_set_passes(PASS_ALL)                              # accepted before the uniforms
    fresh.accum_begin()
    assert _code(lambda: fresh.accum_add(1)) == E_STATE           # before the first set_uniforms
    for kw2 in ({"literal": True}, {"row_rank": 0, "row_world": 2}):
        q = B.RayPass(CFGS["40x36_of_a_ladder"](), device=0, **kw2)
        q.accum_set_passes(PASS_ALL)                              # validates and stores: accepted
        assert _code(q.accum_begin) == E_STATE and q.accum_passes() == 0, kw2
        assert _code(lambda: q.accum_read_pass(PASS_COVERAGE)) == E_STATE, kw2
    rp.set_mesh_lensing(1)                                        # lensing without BHRAY_LENS_RAYS: refused as before
    rp.accum_set_passes(PASS_ALL); rp.accum_begin()
    assert _code(lambda: rp.accum_add(1)) == E_STATE
    rp.close()


# ---- 10. hosts -----------------------------------------------------------------------------------------------------------------
def test_render_still_takes_the_passes():
    r = B.Renderer(CFGS["40x36_of_a_ladder"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    plain = r.render_still(samples=4)
    still = r.render_still(samples=4, passes="coverage,escape")
    assert np.array_equal(_bits(still), _bits(plain)) and r.ray_pass.accum_passes() == PASS_COVERAGE | PASS_ESCAPE
    rp = B.RayPass(CFGS["40x36_of_a_ladder"](), device=0)
    rp.set_textures(*T.textures())
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    want = _still(rp, [4], PASS_COVERAGE | PASS_ESCAPE)
    for name in ("coverage", "escape"):
        got = r.still_pass(name)
        assert got.shape == (36, 40, 4) and np.array_equal(_bits(got.reshape(-1, 4)), _bits(want[name])), name
        assert np.array_equal(_bits(r.still_pass(PASSES[name])), _bits(got))
    assert _code(lambda: r.still_pass("geometry")) == E_INVALID
    with pytest.raises(ValueError):
        r.still_pass("depth")
    with pytest.raises(ValueError):
        r.render_still(adaptive=B.AdaptiveStill(2, 6, 2, 0.05), passes=PASS_COVERAGE)
    r.render_still(samples=2, passes=["geometry", PASS_POSITION])
    assert r.ray_pass.accum_passes() == PASS_GEOMETRY | PASS_POSITION
    r.render_still(samples=2)
    assert r.ray_pass.accum_passes() == 0, "a still without passes carries none"


def test_cpp_host_writes_the_passes(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "still.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp", "4", "--passes", "coverage,escape"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "40x37"
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    still = r2.render_still(samples=4, passes=PASS_COVERAGE | PASS_ESCAPE)
    assert np.array_equal(_bits(np.fromfile(out, dtype=np.float32).reshape(37, 40, 4)), _bits(still))
    for name in ("coverage", "escape"):
        got = np.fromfile(str(out) + "." + name, dtype=np.float32)
        assert got.size == 40 * 37 * 4
        assert np.array_equal(_bits(got.reshape(37, 40, 4)), _bits(r2.still_pass(name))), f"the C++ host's {name} pass differs from the library's words"
    assert not os.path.exists(str(out) + ".geometry") and not os.path.exists(str(out) + ".position")


# ---- 11. cost ------------------------------------------------------------------------------------------------------------------
def test_the_cost_of_the_passes_at_1080p():
    """One run each after a warm-up, the wall clock around accum_add(4) plus a read of the colour: no bar on the ratio (DESIGN.md §27 quotes a run of this test)."""
    rp = B.RayPass(B.ladder_for_frame((1920, 1080), 3, 4), device=0)
    rp.set_textures(*T.textures(small=False))
    rp.set_uniforms(*T.uniforms(integration_method=1))
    times = {}
    for passes in (0, PASS_ALL, 0, PASS_ALL):                     # the first two are the warm-up (allocations, code objects)
        rp.accum_set_passes(passes)
        rp.accum_begin()
        rp.sync()
        t0 = time.perf_counter()
        rp.accum_add(4)
        colour = rp.accum_read()
        times[passes] = (time.perf_counter() - t0) * 1e3
    assert colour.shape == (1080, 1920, 4) and rp.accum_passes() == PASS_ALL
    cov = rp.accum_read_pass(PASS_COVERAGE)
    assert (cov[..., 3] == 1.0).all() and 0.0 < float(cov[..., 1].mean()) < 1.0, "the disk covers part of the default frame"
    print(f"1920 x 1080, 4 samples, RK: set 0 {times[0]:.2f} ms, BHRAY_PASS_ALL {times[PASS_ALL]:.2f} ms (x{times[PASS_ALL] / times[0]:.3f}), single runs")
    rp.close()
