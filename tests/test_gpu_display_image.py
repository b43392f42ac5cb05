"""-m gpu: the display kernels (bhray_post.hip: bloom_kernel x9, final_kernel, fxaa_kernel) on SUPPLIED images, through
bhray_diag_display_image - the launch_display the three product callers run, with no ctx in front of it.  A rendered sky image has alpha 1,
no negative channel, hardly a denormal and no HDR peak; the images here do.

  a. All 18 cases of tests/golden/wgsl_exec_post.npz - what the reference's own bloom_down / bloom_up / mix / hdr / fxaa.wgsl gave when
     executed: the device's RGBA8 bytes, its bloom levels 0 to 8 and its tone-mapped image equal the stored arrays in every word.  No
     restatement is in that chain.
  b. The same bytes equal tests/post_ref.py's: the anchor of c. to e., which have no executed fixture.
  c. A frame whose every bloom level is binary16 denormals: levels, tone image and bytes equal post_ref's stage by stage.
  d. fxaa_kernel's RGBA8 store over every non-negative finite binary16 colour and every binary16 alpha pattern (NaN, +-inf, negatives).
  e. A NaN, then an infinity, in one texel of a sky image: the bytes equal post_ref's (DESIGN.md §10 rule 4; outside the executed pin).
  f. The supplied-image path is the product path: display_image(read_sky()) is read_display(), and the accumulation's display read likewise.
  g. Every refusal is a code, and a valid call after it still gives a.'s bytes.

Every comparison prints how many words it compared and how many differed (-s shows it).  Frames are 131 x 70 at the most, 256 x 256 in d.;
f. runs the device alone, on the ladder frame the other display tests use.
"""
import functools
import os

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import layouts
from oracle import wgsl_exec_post as WP
from tests import common as T
from tests import post_ref as P
from tests import test_gpu_display as D
from tests.test_wgsl_post_pin import CASES, SYNTH, sky_of, stored, uniforms_of

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_INVALID, E_NO_DEVICE = -1, -2
ONE16 = 0x3C00


@functools.lru_cache(maxsize=None)
def _fixtures():
    return np.load(os.path.join(GOLD, "wgsl_exec_post.npz")), np.load(os.path.join(GOLD, "wgsl_exec.npz"))


def _case(name):
    g, r = _fixtures()
    fb, mb, fx, mixr = uniforms_of(g, name)
    return np.ascontiguousarray(sky_of(g, r, name)), fb, mb, fx, mixr


@functools.lru_cache(maxsize=None)
def _device(name):
    """one run of the device per case, shared by a. and b.: (rgba8, [level 0..8], tone), the last two as uint16 words"""
    sky16, fb, mb, _, _ = _case(name)
    return B.display_image(sky16, fb, mb, stages=True)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _same(what, stage, got, want):
    """every word (or byte) of a stage; the failure names the stage and the first five (y, x)"""
    got, want = _words(got), _words(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {stage}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    bad = got != want
    print(f"{what}: {stage}: {bad.size} words compared, {int(bad.sum())} differ")
    px = bad.any(axis=-1)
    assert not px.any(), f"{what}: first differing stage {stage}: {int(px.sum())} pixels, first at (y, x) {np.argwhere(px)[:5].tolist()}"
    return bad.size


def _ref_stages(sky16, fx, mixr):
    """tests/post_ref.py stage by stage, as tests/test_wgsl_post_pin.py chains it: ([level 0..9] as (h, w, 4) words with alpha 1.0, the tone
    image's words, FXAA's f32 output, the RGBA8 bytes)"""
    s = np.asarray(sky16, np.float16).astype(np.float32)
    H, W = s.shape[:2]
    img, levels = s[..., :3], []
    for i, (w, h) in enumerate(P.bloom_sizes(W, H)):
        img = P.bloom_down(img, w, h) if i < 5 else P.bloom_up(img, w, h)
        lv = np.full((h, w, 4), ONE16, np.uint16)
        lv[..., :3] = img.astype(np.float16).view(np.uint16)
        levels.append(lv)
    tone = P.hdr(P.mix(s, img, mixr))
    out = P.fxaa(tone, fx)
    rgba8 = np.empty(out.shape, np.uint8)
    rgba8[..., :3] = P.srgb_encode(out[..., :3])
    rgba8[..., 3] = P.unorm8(out[..., 3])
    return levels, tone.astype(np.float16).view(np.uint16), out, rgba8


# ---- a. the executed shaders ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_a_device_equals_the_executed_shaders_in_every_word(name):
    g, _ = _fixtures()
    sky16 = _case(name)[0]
    H, W = sky16.shape[:2]
    got8, levels, tone = _device(name)
    sizes = B.bloom_sizes(W, H)
    assert [lv.shape for lv in levels] == [(h, w, 4) for w, h in sizes[:9]] and tone.shape == (H, W, 4)
    # in launch order, so that the first stage named is the first that went wrong
    for i, lv in enumerate(levels):
        want = stored(g, name, f"level{i}")
        if want is not None:
            assert (want[..., 3] == ONE16).all()
            _same(name, f"bloom level {i} ({sizes[i][0]}x{sizes[i][1]})", lv, want)
    want = stored(g, name, "hdr")
    if want is not None:
        _same(name, "hdr (the tone-mapped image)", tone, want)
    _same(name, "RGBA8 store", got8, g[f"{name}.rgba8"])


def test_a_the_fixture_has_stage_targets_for_the_cases_the_issue_counts():
    g, _ = _fixtures()
    with_levels = [n for n in CASES if stored(g, n, "level0") is not None]
    with_hdr = [n for n in CASES if stored(g, n, "hdr") is not None]
    assert set(SYNTH) - {"s131x70"} <= set(with_levels) and len(with_levels) >= 15 and len(with_hdr) == len(CASES) == 18
    alpha = np.unique(np.concatenate([g[f"{n}.rgba8"][..., 3].reshape(-1) for n in SYNTH]))
    assert {0, 255} <= set(alpha.tolist()) and len(alpha) >= 4                                            # unorm_byte beyond alpha 1.0


# ---- b. the restatement at the same inputs -----------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_b_device_equals_post_ref_at_the_same_inputs(name):
    sky16, _, _, fx, mixr = _case(name)
    _same(name, "RGBA8 against post_ref", _device(name)[0], P.post_ref(sky16, fx, mixr))


# ---- c. denormal results -------------------------------------------------------------------------------
def _denormal_frame():
    rng = np.random.default_rng(7)
    W, H = 63, 35
    sky = np.ones((H, W, 4), np.float16)
    sky[..., :3] = (10.0 ** rng.uniform(-7.5, -4.0, (H, W, 3))).astype(np.float16)
    zero = rng.permutation(W * H).reshape(H, W) < (W * H) // 5
    sky[zero, :3] = 0
    return sky


def test_c_bloom_levels_of_binary16_denormals_equal_post_ref_stage_by_stage():
    sky16 = _denormal_frame()
    assert (sky16[..., :3] == 0).all(axis=-1).sum() == (63 * 35) // 5 and (sky16[..., 3] == 1).all()
    df, dm = B.post_defaults()
    fx, mixr = D._fxaa_tuple(df), np.float32(dm.mix_ratio)
    levels, tone, _, rgba8 = _ref_stages(sky16, fx, mixr)
    for i in range(9):                                              # the condition, on the restatement's stages alone
        w = levels[i][..., :3] & 0x7FFF
        nonzero, denormal = int((w != 0).sum()), int(((w != 0) & (w < 0x0400)).sum())
        print(f"denormal frame: level {i}: {nonzero} non-zero words, {denormal} denormal")
        assert nonzero > 0 and 2 * denormal >= nonzero, f"level {i}: {denormal} of {nonzero} non-zero words are denormals"
    got8, got_levels, got_tone = B.display_image(sky16, stages=True)
    for i in range(9):
        _same("denormal frame", f"bloom level {i}", got_levels[i], levels[i])
    _same("denormal frame", "hdr (the tone-mapped image)", got_tone, tone)
    _same("denormal frame", "RGBA8 store", got8, rgba8)


# ---- d. the RGBA8 store over all of binary16 -----------------------------------------------------------
def _all_of_binary16(multiplier):
    """256 x 256 tone-mapped image and the RGBA8 bytes post_ref's FXAA and store give for it: red every non-negative finite binary16 (twice
    and a bit), green the same in reverse, blue 1.0, alpha (pattern * multiplier) % 65536 - every bit pattern once, the multiplier being odd"""
    pattern = np.arange(65536, dtype=np.uint32).reshape(256, 256)
    tone16 = np.empty((256, 256, 4), np.uint16)
    tone16[..., 0] = pattern % 0x7C00
    tone16[..., 1] = 0x7BFF - pattern % 0x7C00
    tone16[..., 2] = ONE16
    tone16[..., 3] = (pattern * multiplier) % 65536
    assert len(np.unique(tone16[..., 0])) == 31744 == len(np.unique(tone16[..., 1])) and len(np.unique(tone16[..., 3])) == 65536
    fx = (np.float32(3.0e38), np.float32(0.0), 12, np.float32(0.75))            # every pixel leaves at the early exit
    tone = tone16.view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        out = P.fxaa(tone, fx)
        alpha = P.unorm8(out[..., 3])
    assert np.array_equal(out[..., :3].view(np.uint32), tone[..., :3].view(np.uint32)), "precondition: fxaa passes r, g, b through"
    want = np.empty((256, 256, 4), np.uint8)
    want[..., :3] = P.srgb_encode(out[..., :3])
    want[..., 3] = alpha
    assert np.array_equal(want[..., :3], WP.srgb8(out[..., :3])), "the threshold table against the binary64 definition"
    assert len(np.unique(want[..., :3])) == 256
    return tone16, want


def test_d_rgba8_store_of_every_binary16_colour_and_alpha_pattern():
    """Both sides are powers of two, so the fragment coordinates are exact and the bilinear weights are 0: r, g, b pass through.  Alpha does
    not quite: `a * (1 - 0) + b * 0` is NaN where a neighbour to the right, below or diagonally below holds NaN or an infinity, so 8 160 of the
    65 536 alphas come out NaN (byte 0) for 2 046 NaN inputs.  With the multiplier 40503 every pattern of alpha byte 13 has such a diagonal
    neighbour (pattern + 257 -> word + 0xD537, which is 0xFF7D..0xFFFD) and the expectation holds 255 alpha bytes; the second image (multiplier
    1: the non-finite words fill whole rows) holds all 256.  Both are run."""
    seen = set()
    for multiplier in (40503, 1):
        tone16, want = _all_of_binary16(multiplier)
        alpha = set(np.unique(want[..., 3]).tolist())
        print(f"all of binary16, alpha multiplier {multiplier}: {len(alpha)} alpha bytes in the expectation, missing {sorted(set(range(256)) - alpha)}")
        assert len(alpha) >= 255
        seen |= alpha
        got = B.display_image(tone16, layouts.BhrayFxaaDetails(3.0e38, 0.0, 12, 0.75), fxaa_only=True)
        _same(f"all of binary16, alpha multiplier {multiplier}", "RGBA8 store", got, want)
    assert seen == set(range(256)) and len(alpha) == 256


# ---- e. non-finite input ---------------------------------------------------------------------------------
# (x, y) of the texel.  bloom_down fetches NEAREST at 13 taps whose column and row offsets have the same parity, and 131 x 70 -> 65 x 35 puts every
# tap's centre on an odd column and an odd row: texel (65, 33) is a centre tap and reaches every level, texel (64, 33) is no tap of any pixel and
# never enters the bloom chain - it reaches the frame through mix alone.
@pytest.mark.parametrize("texel", [(65, 33), (64, 33)], ids=["a_bloom_tap", "no_bloom_tap"])
@pytest.mark.parametrize("word", [0x7E00, 0x7C00], ids=["nan", "inf"])
def test_e_one_non_finite_texel_gives_post_refs_bytes(word, texel):
    sky16 = _case("s131x70")[0].copy()
    assert sky16.shape == (70, 131, 4)
    sky16.view(np.uint16)[texel[1], texel[0], 1] = word
    df, dm = B.post_defaults()
    with np.errstate(all="ignore"):
        levels, _, _, want = _ref_stages(sky16, D._fxaa_tuple(df), np.float32(dm.mix_ratio))
    spread = not np.isfinite(levels[3].view(np.float16)).all()                       # the 8 x 4 level
    assert spread == (texel == (65, 33))
    got = B.display_image(sky16)
    lit = lambda a: int((a[..., :3] != 0).any(axis=-1).sum())       # noqa: E731
    print(f"green of texel {texel} = {word:#06x}: {lit(got)} of {got.shape[0] * got.shape[1]} pixels are not black on the device, {lit(want)} in post_ref")
    assert lit(want) == 0 if spread else lit(want) > 9000
    _same(f"green of texel {texel} = {word:#06x}", "RGBA8 store", got, want)


# ---- f. the supplied-image path is the product path ------------------------------------------------------
def test_f_display_image_of_read_sky_is_read_display():
    rp = D._rp(B.ladder_from_base((72, 41), 3, 3), T.textures(), camera=D.POSE_OUT, method=1)
    rp.render()
    rp.resolve_display()
    want, sky = rp.read_display(), rp.read_sky()
    rp.close()
    assert sky.dtype == np.float16 and len(np.unique(want[..., :3].reshape(-1, 3), axis=0)) > 50
    _same("ladder frame", "display_image(read_sky()) against read_display()", B.display_image(sky), want)


def test_f_display_image_of_the_rounded_mean_is_accum_read_display():
    rp = B.RayPass(B.ladder_from_base((33, 32), 3, 1), device=0)
    rp.set_textures(*T.textures())
    rp.set_uniforms(*T.uniforms(camera=B.Camera(), integration_method=1))
    rp.accum_begin()
    rp.accum_add(4)
    mean, want = rp.accum_read(), rp.accum_read_display()
    rp.close()
    with np.errstate(over="ignore"):
        sky16 = mean.astype(np.float16)                             # nearest even
    assert want.shape == (32, 33, 4)
    _same("33 x 32, 4 samples", "display_image(mean16) against accum_read_display()", B.display_image(sky16), want)


# ---- g. refusals -----------------------------------------------------------------------------------------
def test_g_refusals_are_codes_and_the_next_valid_call_is_unharmed():
    g, _ = _fixtures()
    L = B.lib()
    sky16, fb, mb, _, _ = _case("s32x32")
    want = g["s32x32.rgba8"]
    img = sky16.view(np.uint16)
    n = sum(w * h for w, h in B.bloom_sizes(32, 32)[:9]) + 32 * 32
    stages = np.zeros((n + 1, 4), np.uint16)
    dst = np.zeros((32, 32, 4), np.uint8)
    many = bytes(layouts.BhrayFxaaDetails(0.0156, 0.063, layouts.FXAA_MAX_ITERATIONS + 1, 0.75))
    I, Dst, S = img.ctypes.data, dst.ctypes.data, stages.ctypes.data
    refused = [
        ("NULL image", E_INVALID, (0, None, 32, 32, fb, mb, 0, Dst, None, 0)),
        ("NULL destination", E_INVALID, (0, I, 32, 32, fb, mb, 0, None, None, 0)),
        ("31 x 32", E_INVALID, (0, I, 31, 32, fb, mb, 0, Dst, None, 0)),
        ("32 x 31", E_INVALID, (0, I, 32, 31, fb, mb, 0, Dst, None, 0)),
        ("31 x 32, fxaa only", E_INVALID, (0, I, 31, 32, fb, mb, 1, Dst, None, 0)),
        ("32 x 31, fxaa only", E_INVALID, (0, I, 32, 31, fb, mb, 1, Dst, None, 0)),
        ("iterations above the bound", E_INVALID, (0, I, 32, 32, many, mb, 0, Dst, None, 0)),
        ("iterations above the bound, fxaa only", E_INVALID, (0, I, 32, 32, many, mb, 1, Dst, None, 0)),
        ("flag bit 1", E_INVALID, (0, I, 32, 32, fb, mb, 2, Dst, None, 0)),
        ("flag bit 31", E_INVALID, (0, I, 32, 32, fb, mb, 0x80000000, Dst, None, 0)),
        ("stage buffer one texel short", E_INVALID, (0, I, 32, 32, fb, mb, 0, Dst, S, n - 1)),
        ("stage buffer one texel long", E_INVALID, (0, I, 32, 32, fb, mb, 0, Dst, S, n + 1)),
        ("stage buffer beside the flag", E_INVALID, (0, I, 32, 32, fb, mb, 1, Dst, S, n)),
        ("device -1", E_NO_DEVICE, (-1, I, 32, 32, fb, mb, 0, Dst, None, 0)),
        ("a device past the last", E_NO_DEVICE, (L.bhray_device_count(), I, 32, 32, fb, mb, 0, Dst, None, 0)),
    ]
    for what, code, args in refused:
        assert L.bhray_diag_display_image(*args) == code, what
        assert (dst == 0).all() and (stages == 0).all(), f"{what}: the refusal wrote"
        got = B.display_image(sky16, fb, mb)
        bad = (got != want).any(axis=-1)
        assert not bad.any(), f"after `{what}`: {int(bad.sum())} pixels differ from the executed shaders, first at (y, x) {np.argwhere(bad)[:5].tolist()}"
    print(f"refusals: {len(refused)} refused calls, each followed by {want.size} bytes compared, 0 differ")
