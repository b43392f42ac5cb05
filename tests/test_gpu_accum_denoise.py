"""-m gpu: denoised stills - a read-time, edge-avoiding a-trous filter over the accumulation image, guided by the still passes (bhray_accum_read_denoised;
DESIGN.md §28).

  1. accum_read_denoised is, in every word, the NumPy restatement (tests/accum_denoise_ref.py) over the device's own accum_read and accum_read_pass images: box and
     tent, iterations 1 .. 5, the guide subsets, accumulations that carry a subset, a fisheye still (zero vectors outside the circle) and a lens still.
  2. accum_read keeps its bits across a denoised read, and an accumulation continued behind one equals an uninterrupted one bit for bit.
  3. accum_read_display_denoised is display_image over the RGBA16F rounding of the denoised mean, byte for byte.
  4. Refusals: the state and argument codes, with nothing changed afterwards.
  5. Quality: a defocused thin-lens still of 4 samples, denoised with the defaults, is closer to the same still at 256 samples than the undenoised one (printed).
  6. Renderer.render_still(denoise=...), save_still(denoise=...) and bhray_render --spp 4 --denoise agree with 1.
  7. Cost at 1920 x 1080: the prepare launch and the five a-trous launches from events, printed (no bar).

The scene and the ctx are tests/test_gpu_accum_passes.py's; the frames are its two and 70 x 37 (three blocks in x at spacing 1, two at spacing 2)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from bhusie_amd.cameras import StillCamera
from bhusie_amd.layouts import PASS_COVERAGE, PASS_GEOMETRY, PASS_POSITION, PASS_ESCAPE, PASS_ALL
from tests import accum_denoise_ref as DR
from tests import common as T
from tests import test_gpu_accum_passes as GP

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
BITS = (PASS_COVERAGE, PASS_GEOMETRY, PASS_POSITION, PASS_ESCAPE)
SUBSETS = [sum(c) for n in range(1, 5) for c in itertools.combinations(BITS, n)]
CFGS = dict(GP.CFGS)
CFGS["70x37_of_a_ladder"] = lambda: B.ladder_from_base((24, 13), 3, 2)
S4 = 4
# the quality still: tests/test_gpu_accum_passes.py's LENS_CAM through a wide lens focused far in front of the disk, so that every pixel's four lens points see
# different things - chosen on the CPU
QUALITY_FRAME, QUALITY_LENS = (128, 72), StillCamera.pinhole(lens_radius=0.8, focus_distance=4.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _params(iterations=3, guides=0, **sig):
    """sigmas that leave every term something to do in the scene of the passes' tests (the defaults have their own test: the quality)"""
    p = {"iterations": iterations, "guides": guides, "sigma_colour": 0.4, "sigma_coverage": 0.8, "sigma_closest": 3.0, "sigma_position": 6.0, "sigma_escape": 0.7}
    p.update(sig)
    return p


def _still(rp, samples=S4, passes=PASS_ALL, filt=None, camera=None):
    rp.accum_set_filter(filt)
    rp.accum_set_camera(camera)
    rp.accum_set_passes(passes)
    rp.accum_begin()
    rp.accum_add(samples)


def _inputs(rp):
    """C_0 and the guide means exactly as the reads deliver them"""
    return rp.accum_read(), {bit: rp.accum_read_pass(bit) for bit in BITS if rp.accum_passes() & bit}


def _assert_words(got, want, what):
    differ = (_bits(got) != _bits(want))
    n = int(differ.sum())
    print(f"{what}: {n} of {differ.size} words differ")
    if n:
        y, x, ch = np.argwhere(differ)[0]
        raise AssertionError(f"{what}: {n} of {differ.size} words differ from the restatement; the first at pixel ({x}, {y}) channel {ch}: {got[y, x, ch]!r} != {want[y, x, ch]!r}")


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "tent_1.5"], ids=["box", "tent_1.5"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_denoised_read_is_the_restatement_at_every_iteration_count(shape, filt):
    rp = GP._ctx(CFGS[shape]())
    _still(rp, filt=GP.FILTERS[filt][0] if filt else None)
    colour, guides = _inputs(rp)
    assert sorted(guides) == list(BITS) and (colour[..., 3] == 1.0).all()
    changed = 0
    for iterations in (1, 2, 3, 4, 5):
        p = _params(iterations)
        got = rp.accum_read_denoised(B.StillDenoise(**p))
        assert got.shape == colour.shape and got.dtype == np.float32
        _assert_words(got, DR.denoise(colour, guides, p), f"{shape} {filt or 'box'}, {iterations} iterations")
        changed += int((_bits(got) != _bits(colour)).any(axis=-1).sum())
    assert changed > colour.shape[0] * colour.shape[1], "the filter must have something to do in this scene"
    rp.close()


def test_every_guide_subset_is_the_restatement():
    rp = GP._ctx(CFGS["70x37_of_a_ladder"]())
    _still(rp)
    colour, guides = _inputs(rp)
    results = {}
    for subset in SUBSETS:
        p = _params(3, guides=subset)
        results[subset] = rp.accum_read_denoised(B.StillDenoise(**p))
        _assert_words(results[subset], DR.denoise(colour, guides, p), f"guides 0x{subset:x} of BHRAY_PASS_ALL")
    assert np.array_equal(_bits(rp.accum_read_denoised(B.StillDenoise(**_params(3, guides=0)))), _bits(results[PASS_ALL])), "guides 0 is the whole set"
    assert len({results[s].tobytes() for s in SUBSETS}) >= 8, "the guides must matter in this scene"
    # an accumulation that carries a subset: guides 0 is that subset, and the planes outside it are neither there nor read
    for carried in (PASS_COVERAGE | PASS_ESCAPE, PASS_GEOMETRY, PASS_POSITION | PASS_GEOMETRY):
        _still(rp, passes=carried)
        c2, g2 = _inputs(rp)
        assert sum(g2) == carried and np.array_equal(_bits(c2), _bits(colour)), "the colour keeps its bits whatever the set"
        got = rp.accum_read_denoised(B.StillDenoise(**_params(3, guides=0)))
        _assert_words(got, DR.denoise(c2, g2, _params(3, guides=0)), f"an accumulation that carries 0x{carried:x}, guides 0")
        assert np.array_equal(_bits(got), _bits(results[carried])), "the same guides out of a larger set give the same image"
    rp.close()


@pytest.mark.parametrize("kind", ["fisheye", "lens"])
def test_a_still_camera(kind):
    still = {"fisheye": StillCamera.fisheye(3.4), "lens": StillCamera.pinhole(lens_radius=0.3, focus_distance=12.0)}[kind]
    rp = GP._ctx(CFGS["40x36_of_a_ladder"](), 1, camera=GP.LENS_CAM if kind == "lens" else GP.NEAR, mesh=False)
    _still(rp, camera=still)
    colour, guides = _inputs(rp)
    if kind == "fisheye":                                         # 40 x 36: the circle (diameter 36) is smaller than the frame is wide
        outside = ~guides[PASS_ESCAPE][..., 0:3].any(axis=-1) & ~guides[PASS_COVERAGE][..., 0:3].any(axis=-1) & ~colour[..., 0:3].any(axis=-1)
        assert int(outside.sum()) >= 40, "pixels outside the image circle: zero vectors in every pass"
    for iterations in (1, 3, 5):
        p = _params(iterations)
        got = rp.accum_read_denoised(B.StillDenoise(**p))
        _assert_words(got, DR.denoise(colour, guides, p), f"{kind}, {iterations} iterations")
    rp.close()


# ---- 2. no accumulation state changes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, "tent_1.5"], ids=["box", "tent_1.5"])
def test_a_denoised_read_changes_no_accumulation_state(filt):
    f = GP.FILTERS[filt][0] if filt else None
    rp = GP._ctx(CFGS["40x36_of_a_ladder"]())
    _still(rp, samples=5, filt=f)
    whole, whole_guides = _inputs(rp)
    rp.accum_set_passes(PASS_ALL)
    rp.accum_begin()
    rp.accum_add(2)
    before, before_guides = _inputs(rp)
    first = rp.accum_read_denoised(B.StillDenoise(**_params(5)))
    rp.accum_read_display_denoised()
    assert rp.accum_samples() == 2 and rp.accum_passes() == PASS_ALL
    after, after_guides = _inputs(rp)
    assert np.array_equal(_bits(after), _bits(before)), "accum_read changed across a denoised read"
    for bit in BITS:
        assert np.array_equal(_bits(after_guides[bit]), _bits(before_guides[bit])), f"pass 0x{bit:x} changed across a denoised read"
    assert np.array_equal(_bits(rp.accum_read_denoised(B.StillDenoise(**_params(5)))), _bits(first)), "the denoised read is a pure function"
    rp.accum_add(3)                                               # the accumulation goes on
    cont, cont_guides = _inputs(rp)
    assert np.array_equal(_bits(cont), _bits(whole)), "2 samples, a denoised read, 3 samples: not the uninterrupted 5"
    for bit in BITS:
        assert np.array_equal(_bits(cont_guides[bit]), _bits(whole_guides[bit]))
    rp.close()


# ---- 3. the display read -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_display_read_is_the_display_pass_over_the_binary16_denoised_mean(shape):
    rp = GP._ctx(CFGS[shape]())
    _still(rp)
    for d in (None, B.StillDenoise(**_params(1)), B.StillDenoise(**_params(4, guides=PASS_COVERAGE | PASS_ESCAPE))):
        mean = rp.accum_read_denoised(d)
        disp = rp.accum_read_display_denoised(d)
        assert disp.shape == mean.shape and disp.dtype == np.uint8
        with np.errstate(over="ignore"):
            want = B.display_image(mean.astype(np.float16))       # nearest even
        assert np.array_equal(disp, want), "the denoised display read differs from display_image over the binary16 denoised mean"
    plain = rp.accum_read_display()
    assert not np.array_equal(plain, disp), "the denoised display image must differ from the plain one"
    assert np.array_equal(rp.accum_read_display(), plain)
    rp.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    rp = GP._ctx(CFGS["40x36_of_a_ladder"]())
    code = GP._code
    for read in (rp.accum_read_denoised, rp.accum_read_display_denoised, rp.accum_denoise_times):
        assert code(read) == E_STATE, "before accum_begin"
    rp.accum_set_passes(0)
    rp.accum_begin(); rp.accum_add(2)
    for read in (rp.accum_read_denoised, rp.accum_read_display_denoised, rp.accum_denoise_times):
        assert code(read) == E_STATE, "an accumulation whose pass set is 0"
    plain = rp.accum_read()
    rp.accum_begin()
    rp.accum_add_adaptive(min_samples=2, max_samples=6, round_samples=2, tolerance=0.05, dark=0.01)
    for read in (rp.accum_read_denoised, rp.accum_read_display_denoised):
        assert code(read) == E_STATE, "an adaptive accumulation"
    _still(rp, samples=2, passes=PASS_COVERAGE | PASS_ESCAPE)
    before, guides = _inputs(rp)
    assert np.array_equal(_bits(before), _bits(plain))
    good = rp.accum_read_denoised()
    bad = [dict(iterations=0), dict(iterations=6), dict(guides=PASS_GEOMETRY), dict(guides=PASS_ALL), dict(guides=0x10), dict(sigma_colour=0.0),
           dict(sigma_coverage=-1.0), dict(sigma_closest=float("nan")), dict(sigma_position=float("inf")), dict(sigma_escape=-0.0)]
    for kw in bad:
        d = B.StillDenoise(**kw)
        assert code(lambda: rp.accum_read_denoised(d)) == E_INVALID, kw
        assert code(lambda: rp.accum_read_display_denoised(d)) == E_INVALID, kw
    st = B.StillDenoise().struct()
    st.struct_size = 28
    assert code(lambda: rp.accum_read_denoised(st)) == E_INVALID, "a wrong struct_size"
    L = B.lib()
    out = np.zeros((36, 40, 4), np.float32)
    assert L.bhray_accum_read_denoised(rp._h, None, None, 40 * 16) == E_INVALID and L.bhray_accum_read_denoised(rp._h, None, out.ctypes.data, 40 * 16 - 1) == E_INVALID
    assert L.bhray_accum_read_denoised(None, None, out.ctypes.data, 40 * 16) == E_INVALID
    assert rp.accum_samples() == 2 and rp.accum_passes() == PASS_COVERAGE | PASS_ESCAPE
    assert np.array_equal(_bits(rp.accum_read()), _bits(before)) and np.array_equal(_bits(rp.accum_read_denoised()), _bits(good)), "a refused read changed something"
    rp.close()
    small = GP._ctx(B.ladder_from_base((24, 14), 3, 1))           # below the display pass's 32 x 32
    _still(small, samples=1)
    assert code(small.accum_read_display_denoised) == E_INVALID
    c, g = _inputs(small)
    _assert_words(small.accum_read_denoised(B.StillDenoise(**_params(5))), DR.denoise(c, g, _params(5)), "24 x 14, where spacing 8 and 16 reach past the frame")
    small.close()
    for kw2 in ({"literal": True}, {"row_rank": 0, "row_world": 2}):
        q = B.RayPass(CFGS["40x36_of_a_ladder"](), device=0, **kw2)
        assert code(q.accum_read_denoised) == E_STATE, kw2


# ---- 5. quality ----------------------------------------------------------------------------------------------------------------
def _compressed_error(a, ref):
    x, y = a[..., 0:3].astype(np.float64), ref[..., 0:3].astype(np.float64)
    return float(((x / (1.0 + x) - y / (1.0 + y)) ** 2).mean())


def test_a_denoised_lens_still_of_4_samples_is_closer_to_256_samples_than_the_plain_one():
    """The bar is the issue's: the denoised error strictly below the undenoised one.  On the CPU (the C oracle over cameras.still_rays, the restatement with the
    coverage and escape guides the oracle's results give) the ratio was 0.109; a run on an MI355X with all four guides printed 0.112."""
    rp = GP._ctx(B.ladder_for_frame(QUALITY_FRAME, 3, 2), 1, camera=GP.LENS_CAM, mesh=False)
    _still(rp, samples=256, passes=0, camera=QUALITY_LENS)       # the yardstick: pre-existing code only
    ref = rp.accum_read()
    _still(rp, samples=4, camera=QUALITY_LENS)
    plain = rp.accum_read()
    denoised = rp.accum_read_denoised()                           # the defaults
    assert np.isfinite(ref).all() and np.isfinite(denoised).all() and (denoised[..., 3] == 1.0).all()
    e_plain, e_denoised = _compressed_error(plain, ref), _compressed_error(denoised, ref)
    print(f"{QUALITY_FRAME[0]} x {QUALITY_FRAME[1]} lens still (radius 0.8, focus 4), 4 against 256 samples: mean square error of c / (1 + c) undenoised {e_plain:.4e}, "
          f"denoised {e_denoised:.4e}, ratio {e_denoised / e_plain:.3f}")
    assert e_denoised < e_plain
    rp.close()


# ---- 6. hosts ------------------------------------------------------------------------------------------------------------------
def test_render_still_and_save_still_take_the_denoiser(tmp_path):
    from PIL import Image
    r = B.Renderer(CFGS["40x36_of_a_ladder"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    plain = r.render_still(samples=4)
    d = B.StillDenoise(**_params(3))
    still = r.render_still(samples=4, denoise=d)
    assert r.ray_pass.accum_passes() == PASS_ALL, "a denoise request with passes == 0 switches on all four"
    colour, guides = _inputs(r.ray_pass)
    assert np.array_equal(_bits(colour), _bits(plain))
    _assert_words(still, DR.denoise(colour, guides, _params(3)), "render_still(denoise=...)")
    assert np.array_equal(_bits(r.render_still(samples=4, denoise=True)), _bits(r.ray_pass.accum_read_denoised())), "True: the library's defaults"
    sub = r.render_still(samples=4, passes="coverage,escape", denoise=d)
    assert r.ray_pass.accum_passes() == PASS_COVERAGE | PASS_ESCAPE
    _assert_words(sub, DR.denoise(colour, {b: guides[b] for b in (PASS_COVERAGE, PASS_ESCAPE)}, _params(3)), "render_still(passes=..., denoise=...)")
    assert np.array_equal(_bits(r.render_still(samples=4, denoise=False)), _bits(plain)) and r.ray_pass.accum_passes() == 0
    with pytest.raises(ValueError):
        r.render_still(adaptive=B.AdaptiveStill(2, 6, 2, 0.05), denoise=d)
    path = tmp_path / "still.png"
    r.save_still(path, samples=4, denoise=d)
    want = r.ray_pass.accum_read_display_denoised(d)
    want[..., 3] = 255
    assert np.array_equal(np.asarray(Image.open(path).convert("RGBA")), want)


def test_cpp_host_writes_the_denoised_still(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    base = [exe, None, "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp", "4"]
    for extra, kw in ((["--denoise"], dict(denoise=True)), (["--denoise", "4", "--passes", "coverage,escape"], dict(denoise=B.StillDenoise(iterations=4), passes="coverage,escape"))):
        out = tmp_path / ("still%d.f32" % len(extra))
        cmd = list(base)
        cmd[1] = str(out)
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == "40x37"
        still = r2.render_still(samples=4, **kw)
        assert np.array_equal(_bits(np.fromfile(out, dtype=np.float32).reshape(37, 40, 4)), _bits(still)), f"{extra}: the C++ host's denoised still differs from the library's words"
        assert not np.array_equal(_bits(still), _bits(r2.ray_pass.accum_read()))
        assert os.path.exists(str(out) + ".coverage") == ("--passes" in extra) and not os.path.exists(str(out) + ".geometry")
    r = subprocess.run([exe, str(tmp_path / "x.f32"), "--denoise"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--spp" in r.stderr


# ---- 7. cost -------------------------------------------------------------------------------------------------------------------
def test_the_cost_of_the_denoiser_at_1080p():
    """One run after a warm-up, device time between events around each launch: no bar (DESIGN.md §28 quotes a run of this test)."""
    rp = B.RayPass(B.ladder_for_frame((1920, 1080), 3, 4), device=0)
    rp.set_textures(*T.textures(small=False))
    rp.set_uniforms(*T.uniforms(integration_method=1))
    _still(rp)
    d = B.StillDenoise(iterations=5)
    rp.accum_denoise_times(d)                                     # the warm-up: allocations, code objects
    ms = rp.accum_denoise_times(d)
    assert len(ms) == 6 and all(v > 0.0 for v in ms)
    out = rp.accum_read_denoised(d)
    assert out.shape == (1080, 1920, 4) and np.isfinite(out).all()
    print("1920 x 1080, 4 samples, all four guides, 5 iterations, one run: prepare %.3f ms; a-trous at spacing 1, 2, 4, 8, 16: %s ms; total %.3f ms"
          % (ms[0], ", ".join("%.3f" % v for v in ms[1:]), sum(ms)))
    rp.close()
