"""CPU: the display pass's host surface (symbols, uniform layouts, defaults, bloom sizes, argument checks) and known-answer tests of
tests/post_ref.py, the NumPy restatement of bloom_down / bloom_up / mix / hdr / fxaa.wgsl that the GPU tests hold the kernels to
(DESIGN.md §10)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import layouts

from . import post_ref as P

NEW = ("bhray_post_defaults", "bhray_bloom_sizes", "bhray_set_post_uniforms", "bhray_resolve_display", "bhray_read_display",
       "bhray_read_display_async", "bhray_display_device_ptr")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_display_symbols_are_exported_declared_and_bound():
    L = B.lib()
    hdr = open(os.path.join(ROOT, "include", "bhray.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in layouts.SYMBOLS, name
        assert "%s(" % name in hdr, name
    assert L.bhray_version() == (0 << 16) | 5


def test_uniform_blocks_are_the_reference_layouts():
    # FXAADetailsUniform (fxaa_pipline.rs:76-83) and MixDetails (mix_pipeline.rs:5-7)
    assert C.sizeof(layouts.BhrayFxaaDetails) == 16 and C.sizeof(layouts.BhrayMixDetails) == 4
    assert [(n, getattr(layouts.BhrayFxaaDetails, n).offset) for n, _ in layouts.BhrayFxaaDetails._fields_] == \
        [("edge_threshold_min", 0), ("edge_threshold_max", 4), ("iterations", 8), ("subpixel_quality", 12)]
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_fxaa_details, 16)" in src and "SZ(bhray_mix_details, 4)" in src


def test_post_defaults_are_the_bytes_renderer_render_uploads():
    f, m = B.post_defaults()
    assert bytes(f) == struct.pack("<ffif", 0.0156, 0.063, 12, 0.75)        # EdgeThresholdMin/Max::Ultra, 12, 0.75 (mod.rs:290-295)
    assert bytes(m) == struct.pack("<f", 0.7)                                # mod.rs:258-260
    assert (f.edge_threshold_min, f.edge_threshold_max, f.iterations, f.subpixel_quality) == P.FXAA_DEFAULT
    assert np.float32(m.mix_ratio) == P.MIX_DEFAULT


def test_bloom_sizes_follow_the_reference_float_halving():
    assert B.bloom_sizes(1918, 1081) == [(959, 540), (479, 270), (239, 135), (119, 67), (59, 33),
                                         (119, 67), (239, 135), (479, 270), (959, 540), (1918, 1081)]
    assert B.bloom_sizes(1920, 1080) == [(960, 540), (480, 270), (240, 135), (120, 67), (60, 33),
                                         (120, 67), (240, 135), (480, 270), (960, 540), (1920, 1080)]
    for w, h in ((256, 256), (32, 32), (3840, 2160), (1945, 1081), (208, 118), (33, 4097)):
        s = B.bloom_sizes(w, h)
        assert s == P.bloom_sizes(w, h) and s[-1] == (w, h)
    for w, h in ((31, 1080), (1920, 31), (0, 0), (1, 1)):
        with pytest.raises(B.BhrayError) as e:
            B.bloom_sizes(w, h)
        assert e.value.code == -1
        with pytest.raises(ValueError):
            P.bloom_sizes(w, h)


def test_null_and_bad_arguments_are_invalid():
    L = B.lib()
    w, h = (C.c_uint32 * 10)(), (C.c_uint32 * 10)()
    assert L.bhray_bloom_sizes(1920, 1080, None, h) == -1 and L.bhray_bloom_sizes(1920, 1080, w, None) == -1
    assert L.bhray_post_defaults(None, None) == -1
    f, m = layouts.BhrayFxaaDetails(), layouts.BhrayMixDetails()
    assert L.bhray_post_defaults(C.byref(f), None) == 0 and f.iterations == 12
    assert L.bhray_post_defaults(None, C.byref(m)) == 0 and abs(m.mix_ratio - 0.7) < 1e-7
    assert L.bhray_set_post_uniforms(None, bytes(f), bytes(m)) == -1
    assert L.bhray_resolve_display(None) == -1
    assert L.bhray_read_display(None, None, 0) == -1
    t = C.c_uint64()
    assert L.bhray_read_display_async(None, None, 0, C.byref(t)) == -1
    p, n = C.c_void_p(), C.c_size_t()
    assert L.bhray_display_device_ptr(None, C.byref(p), C.byref(n)) == -1


# ---- known answers of the NumPy restatement ------------------------------------------------------------------------------------

def _const(w, h, rgb, a=1.0):
    img = np.empty((h, w, 4), dtype=np.float16)
    img[..., :3] = np.asarray(rgb, dtype=np.float16)
    img[..., 3] = a
    return img


@pytest.mark.parametrize("rgb", [(0.25, 0.25, 0.25), (3.0, 0.5, 0.0625), (0.0, 0.0, 0.0), (100.0, 7.5, 0.001)])
def test_constant_image_goes_through_unchanged_up_to_aces(rgb):
    """down weights sum to 1, up weights to 16/16 (and bilinear taps of a constant are that constant up to an f32 ulp the binary16 store
    absorbs), mix of equal inputs is the input, and FXAA takes its early exit: the result is ACES(c), sRGB-encoded"""
    sky = _const(96, 64, rgb)
    s = sky.astype(np.float32)
    assert np.array_equal(P.bloom(s[..., :3]), s[..., :3])
    tone = P.tone_map(sky)
    want = P.to16(P.aces(np.asarray(rgb, dtype=np.float16).astype(np.float32)))
    assert np.array_equal(tone[..., :3], np.broadcast_to(want, tone[..., :3].shape)) and (tone[..., 3] == 1.0).all()
    out = P.post_ref(sky)
    assert (out[..., :3] == P.srgb_encode(want)).all() and (out[..., 3] == 255).all()


def test_aces_matches_a_float64_evaluation():
    pts = np.array([[0.0, 0.0, 0.0], [0.01, 0.02, 0.03], [0.18, 0.18, 0.18], [0.5, 0.25, 0.125], [1.0, 1.0, 1.0], [2.0, 0.1, 0.7],
                    [4.0, 3.0, 2.0], [1000.0, 1000.0, 1000.0], [0.9, 0.0, 0.05]], dtype=np.float32)
    m1 = P.M1.astype(np.float64); m2 = P.M2.astype(np.float64)
    x = pts.astype(np.float64)
    v = m1[0] * x[:, :1] + m1[1] * x[:, 1:2] + m1[2] * x[:, 2:3]
    q = (v * (v + np.float64(np.float32(0.0245786))) - np.float64(np.float32(0.000090537))) / \
        (v * (np.float64(np.float32(0.983729)) * v + np.float64(np.float32(0.4329510))) + np.float64(np.float32(0.238081)))
    want = np.clip(m2[0] * q[:, :1] + m2[1] * q[:, 1:2] + m2[2] * q[:, 2:3], 0.0, 1.0)
    got = P.aces(pts).astype(np.float64)
    assert np.abs(got - want).max() <= 2e-6, np.abs(got - want).max()
    assert (got[0] == 0.0).all() and (got[-2] == 1.0).all()
    # NaN and infinities go to 0 (clamp is maxNum / minNum)
    assert (P.aces(np.array([[np.nan, 1.0, 1.0], [np.inf, np.inf, np.inf]], dtype=np.float32))[1] == 0.0).all()
    assert P.aces(np.array([[np.nan, 0.0, 0.0]], dtype=np.float32))[0, 0] == 0.0


def _srgb_closed_form(v):
    v = np.asarray(v, dtype=np.float64)
    e = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 0.0), 1.0 / 2.4) - 0.055)
    return np.floor(np.clip(e, 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)


def test_srgb_table_against_the_closed_form_at_every_threshold():
    t = P.srgb_thresholds()
    assert t.dtype == np.float32 and t.shape == (255,) and (np.diff(t) > 0).all()
    k = np.arange(1, 256)
    above = np.nextafter(t, np.float32(np.inf))
    below = np.nextafter(t, np.float32(-np.inf))
    assert (P.srgb_encode(t) == k).all()
    assert (P.srgb_encode(below) == k - 1).all()
    assert (P.srgb_encode(above) == k).all()
    assert (_srgb_closed_form(above) == k).all()
    assert (_srgb_closed_form(below) == k - 1).all()
    assert P.srgb_encode(np.float32(0.0)) == 0 and P.srgb_encode(np.float32(1.0)) == 255 and P.srgb_encode(np.float32(np.nan)) == 0
    assert (P.unorm8(np.array([0.0, 1.0, 0.5, 2.0, -1.0, np.nan], dtype=np.float32)) == [0, 255, 128, 255, 0, 0]).all()


@pytest.mark.parametrize("S", [16, 64, 256])
def test_single_bright_pixel_bloom_is_mirror_symmetric(S):
    """The mirror each pass's taps allow.  Down (nearest; u * S lands on 2t + 1 + k, a texel boundary, and floor picks the texel to its
    right): target t <-> T - 1 - t pairs source s <-> S - s, so a single bright pixel at S / 2 gives a response symmetric in t <-> T - 1 - t.
    Up (bilinear at texel centres +- 0.005 uv): t <-> T - 1 - t pairs s <-> S - 1 - s, so the 2 x 2 block at the centre of an even frame
    blooms symmetrically.  Both responses spread and conserve nothing brighter than the source."""
    src = np.zeros((S, S, 3), dtype=np.float32)
    src[S // 2, S // 2] = 1000.0
    d = P.bloom_down(src, S // 2, S // 2)[..., 0]
    assert np.array_equal(d, d[:, ::-1]) and np.array_equal(d, d[::-1, :]) and (d > 0).sum() == 4 and d.max() < 1000.0
    src = np.zeros((S, S, 3), dtype=np.float32)
    src[S // 2 - 1:S // 2 + 1, S // 2 - 1:S // 2 + 1] = 1000.0
    u = P.bloom_up(src, 2 * S, 2 * S)[..., 0]
    assert np.array_equal(u, u[:, ::-1]) and np.array_equal(u, u[::-1, :]) and (u > 0).sum() > 16 and u.max() <= 1000.0
    # and the whole chain spreads one bright block over the frame
    full = np.zeros((256, 256, 3), dtype=np.float32)
    full[127:129, 127:129] = 1000.0
    assert (P.bloom(full)[..., 0] > 0).sum() > 64 * 64


def test_fxaa_leaves_flat_regions_and_moves_a_hard_edge():
    W, H = 64, 48
    flat = np.full((H, W, 4), 0.5, dtype=np.float32); flat[..., 3] = 1.0
    assert np.array_equal(P.fxaa(flat), flat)
    edge = np.zeros((H, W, 4), dtype=np.float32); edge[..., 3] = 1.0
    yy, xx = np.mgrid[0:H, 0:W]
    edge[(xx * 3 + yy * 2) > 100, :3] = 1.0                 # a slanted hard edge
    out = P.fxaa(edge)
    moved = (out[..., :3] != edge[..., :3]).any(axis=-1)
    near = np.abs((xx * 3 + yy * 2) - 100) <= 5
    assert moved.any() and not moved[~near].any()            # pixels on the edge move, pixels away from it do not
    assert (out[..., 3] == 1.0).all()
    # the search loop runs: with 1 iteration (no loop) some edge pixels end up elsewhere than with 20
    assert not np.array_equal(P.fxaa(edge, (0.0312, 0.125, 1, 0.75)), P.fxaa(edge, (0.0312, 0.125, 20, 0.75)))


# ---- fxaa.wgsl:fs_main, one fragment at a time: a scalar transcription of the shader text, line by line (vec2 as tuples, `select(f, t, c)`
# as written), independent of post_ref's vectorised form.  Sampling: ClampToEdge, Linear, texel centres at +0.5, integer offsets added
# to the texel coordinate after the -0.5 (DESIGN.md §10 rule 3).

f32s = np.float32


def _sample(img, uv, off=(0, 0)):
    h, w = img.shape[:2]
    out = []
    for n, u, o in ((w, uv[0], off[0]), (h, uv[1], off[1])):
        x = f32s(f32s(f32s(u) * f32s(n)) - f32s(0.5))
        x = f32s(x + f32s(o))
        x = f32s(-1.0) if not (x >= -1.0) else x
        x = f32s(n) if x > n else x
        fl = f32s(np.floor(x))
        i0 = min(max(int(fl), 0), n - 1)
        i1 = min(max(int(fl) + 1, 0), n - 1)
        out.append((i0, i1, f32s(x - fl)))
    (x0, x1, fx), (y0, y1, fy) = out
    mix = lambda a, b, t: a * (f32s(1.0) - t) + b * t       # noqa: E731
    return mix(mix(img[y0, x0], img[y0, x1], fx), mix(img[y1, x0], img[y1, x1], fx), fy)


def _select(f, t, c):
    return t if c else f


def _rgb2luma(rgb):
    return f32s(np.sqrt(f32s(f32s(f32s(rgb[0] * f32s(0.299)) + f32s(rgb[1] * f32s(0.587))) + f32s(rgb[2] * f32s(0.114)))))


def _QUALITY(q):
    return f32s({5: 1.5, 6: 2.0, 7: 2.0, 8: 2.0, 9: 2.0, 10: 4.0, 11: 8.0}.get(q, 1.0))


def _fs_main(img, px, py, details, end2_first_step=-1):
    """end2_first_step: the sign of fxaa.wgsl:132's step (`uv2 - offset`: -1); +1 is the textbook FXAA, used only to show the test sees it"""
    emin, emax, iterations, subq = f32s(details[0]), f32s(details[1]), int(details[2]), f32s(details[3])
    H, W = img.shape[:2]
    inv = (f32s(1.0) / f32s(W), f32s(1.0) / f32s(H))
    texCoord = (f32s((px + f32s(0.5)) * inv[0]), f32s((py + f32s(0.5)) * inv[1]))
    centerSample = _sample(img, texCoord)
    lumaCenter = _rgb2luma(centerSample[:3])
    lumaDown = _rgb2luma(_sample(img, texCoord, (0, -1))[:3])
    lumaUp = _rgb2luma(_sample(img, texCoord, (0, 1))[:3])
    lumaLeft = _rgb2luma(_sample(img, texCoord, (-1, 0))[:3])
    lumaRight = _rgb2luma(_sample(img, texCoord, (1, 0))[:3])
    lumaMin = min(lumaCenter, min(min(lumaDown, lumaUp), min(lumaLeft, lumaRight)))
    lumaMax = max(lumaCenter, max(max(lumaDown, lumaUp), max(lumaLeft, lumaRight)))
    lumaRange = f32s(lumaMax - lumaMin)
    if lumaRange < max(emin, f32s(lumaMax * emax)):
        return centerSample
    lumaDownLeft = _rgb2luma(_sample(img, texCoord, (-1, -1))[:3])
    lumaUpRight = _rgb2luma(_sample(img, texCoord, (1, 1))[:3])
    lumaUpLeft = _rgb2luma(_sample(img, texCoord, (-1, 1))[:3])
    lumaDownRight = _rgb2luma(_sample(img, texCoord, (1, -1))[:3])
    lumaDownUp = f32s(lumaDown + lumaUp)
    lumaLeftRight = f32s(lumaLeft + lumaRight)
    lumaLeftCorners = f32s(lumaDownLeft + lumaUpLeft)
    lumaDownCorners = f32s(lumaDownLeft + lumaDownRight)
    lumaRightCorners = f32s(lumaDownRight + lumaUpRight)
    lumaUpCorners = f32s(lumaUpRight + lumaUpLeft)
    m2 = f32s(-2.0)
    edgeHorizontal = f32s(f32s(abs(f32s(m2 * lumaLeft + lumaLeftCorners)) + f32s(abs(f32s(m2 * lumaCenter + lumaDownUp)) * f32s(2.0)))
                          + abs(f32s(m2 * lumaRight + lumaRightCorners)))
    edgeVertical = f32s(f32s(abs(f32s(m2 * lumaUp + lumaUpCorners)) + f32s(abs(f32s(m2 * lumaCenter + lumaLeftRight)) * f32s(2.0)))
                        + abs(f32s(m2 * lumaDown + lumaDownCorners)))
    isHorizontal = edgeHorizontal >= edgeVertical
    stepLength = _select(inv[0], inv[1], isHorizontal)
    luma1 = _select(lumaLeft, lumaDown, isHorizontal)
    luma2 = _select(lumaRight, lumaUp, isHorizontal)
    gradient1 = f32s(luma1 - lumaCenter)
    gradient2 = f32s(luma2 - lumaCenter)
    is1Steepest = abs(gradient1) >= abs(gradient2)
    gradientScaled = f32s(f32s(0.25) * max(abs(gradient1), abs(gradient2)))
    if is1Steepest:
        stepLength = -stepLength
        lumaLocalAverage = f32s(f32s(0.5) * f32s(luma1 + lumaCenter))
    else:
        lumaLocalAverage = f32s(f32s(0.5) * f32s(luma2 + lumaCenter))
    currentUv = list(texCoord)
    offset = [f32s(0.0), f32s(0.0)]
    if isHorizontal:
        currentUv[1] = f32s(currentUv[1] + f32s(stepLength * f32s(0.5)))
        offset[0] = inv[0]
    else:
        currentUv[0] = f32s(currentUv[0] + f32s(stepLength * f32s(0.5)))
        offset[1] = inv[1]
    sub = lambda a, b: (f32s(a[0] - b[0]), f32s(a[1] - b[1]))      # noqa: E731
    add = lambda a, b: (f32s(a[0] + b[0]), f32s(a[1] + b[1]))      # noqa: E731
    scl = lambda a, s: (f32s(a[0] * s), f32s(a[1] * s))             # noqa: E731
    uv1 = sub(currentUv, offset)
    uv2 = add(currentUv, offset)
    lumaEnd1 = f32s(_rgb2luma(_sample(img, uv1)[:3]) - lumaLocalAverage)
    lumaEnd2 = f32s(_rgb2luma(_sample(img, uv2)[:3]) - lumaLocalAverage)
    reached1 = abs(lumaEnd1) >= gradientScaled
    reached2 = abs(lumaEnd2) >= gradientScaled
    reachedBoth = reached1 and reached2
    uv1 = _select(sub(uv1, offset), uv1, reached1)
    uv2 = _select(sub(uv2, offset) if end2_first_step < 0 else add(uv2, offset), uv2, reached2)
    if not reachedBoth:
        for i in range(2, iterations):
            if not reached1:
                lumaEnd1 = f32s(_rgb2luma(_sample(img, uv1)[:3]) - lumaLocalAverage)
            if not reached2:
                lumaEnd2 = f32s(_rgb2luma(_sample(img, uv2)[:3]) - lumaLocalAverage)
            reached1 = abs(lumaEnd1) >= gradientScaled
            reached2 = abs(lumaEnd2) >= gradientScaled
            reachedBoth = reached1 and reached2
            if not reached1:
                uv1 = sub(uv1, scl(offset, _QUALITY(i)))
            if not reached2:
                uv2 = add(uv2, scl(offset, _QUALITY(i)))
            if reachedBoth:
                break
    distance1 = _select(f32s(texCoord[1] - uv1[1]), f32s(texCoord[0] - uv1[0]), isHorizontal)
    distance2 = _select(f32s(uv2[1] - texCoord[1]), f32s(uv2[0] - texCoord[0]), isHorizontal)
    isDirection1 = distance1 < distance2
    distanceFinal = min(distance1, distance2)
    edgeThickness = f32s(distance1 + distance2)
    isLumaCenterSmaller = lumaCenter < lumaLocalAverage
    correctVariation1 = (lumaEnd1 < 0.0) != isLumaCenterSmaller
    correctVariation2 = (lumaEnd2 < 0.0) != isLumaCenterSmaller
    correctVariation = _select(correctVariation2, correctVariation1, isDirection1)
    pixelOffset = f32s(f32s(-distanceFinal / edgeThickness) + f32s(0.5))
    finalOffset = _select(f32s(0.0), pixelOffset, correctVariation)
    lumaAverage = f32s(f32s(1.0 / 12.0) * f32s(f32s(f32s(f32s(2.0) * f32s(lumaDownUp + lumaLeftRight)) + lumaLeftCorners) + lumaRightCorners))
    with np.errstate(invalid="ignore", divide="ignore"):
        subPixelOffset1 = f32s(np.fmin(np.fmax(f32s(abs(f32s(lumaAverage - lumaCenter)) / lumaRange), f32s(0.0)), f32s(1.0)))
    subPixelOffset2 = f32s(f32s(f32s(f32s(m2 * subPixelOffset1) + f32s(3.0)) * subPixelOffset1) * subPixelOffset1)
    subPixelOffsetFinal = f32s(f32s(subPixelOffset2 * subPixelOffset2) * subq)
    finalOffset = max(finalOffset, subPixelOffsetFinal)
    finalUv = list(texCoord)
    if isHorizontal:
        finalUv[1] = f32s(finalUv[1] + f32s(finalOffset * stepLength))
    else:
        finalUv[0] = f32s(finalUv[0] + f32s(finalOffset * stepLength))
    finalColor = _sample(img, finalUv)
    return np.array([finalColor[0], finalColor[1], finalColor[2], centerSample[3]], dtype=np.float32)


def _edge_scene(W=40, H=28):
    """a disc and diagonal stripes of binary16 values in [0, 1]: edges of every orientation, ends reached at different distances"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 4), dtype=np.float32)
    disc = (xx - 13.3) ** 2 + (yy - 12.6) ** 2 < 70.0
    stripes = ((xx + 2 * yy) // 7) % 2 == 0
    img[..., 0] = np.where(disc, 0.9, np.where(stripes, 0.35, 0.05))
    img[..., 1] = np.where(disc, 0.6, np.where(stripes, 0.3, 0.1))
    img[..., 2] = np.where(disc, 0.2, np.where(stripes, 0.8, 0.05))
    img[..., 3] = 1.0
    return P.to16(img)


@pytest.mark.parametrize("details", [P.FXAA_DEFAULT, (0.0078, 0.031, 20, 0.5), (0.0833, 0.25, 6, 1.0), (0.0078, 0.031, 2, 0.75)],
                         ids=["ultra", "extreme_it20", "low_it6", "it2"])
def test_fxaa_restatement_is_the_shader_text_fragment_by_fragment(details):
    """post_ref.fxaa against the scalar transcription of fs_main at every pixel of a frame with edges of every orientation - including the
    first step of the edge search, where fxaa.wgsl:132 moves end 2 by MINUS offset (`uv2 = select(uv2 - offset, uv2, reached2)`), unlike
    the textbook FXAA; the transcription with the textbook step gives other bytes on this frame, so the comparison does see that step"""
    img = _edge_scene()
    H, W = img.shape[:2]
    got = P.fxaa(img, details)
    want = np.stack([np.stack([_fs_main(img, x, y, details) for x in range(W)]) for y in range(H)])
    assert np.array_equal(got, want)
    textbook = np.stack([np.stack([_fs_main(img, x, y, details, end2_first_step=+1) for x in range(W)]) for y in range(H)])
    enc = lambda c: P.srgb_encode(c[..., :3])      # noqa: E731
    assert (enc(textbook) != enc(want)).any(), "the frame does not exercise fxaa.wgsl:132"
