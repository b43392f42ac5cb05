"""CPU: the display-pass restatement (tests/post_ref.py) against images made by EXECUTING the reference's own shader text.

tests/golden/wgsl_exec_post.npz was written by tests/golden/make_golden_wgsl_post.py, which has oracle/wgsl_exec_post.py parse and run
bloom_down / bloom_up / mix / hdr / fxaa.wgsl of the reference tree as the render passes run them (vertex stage, one fragment per pixel);
nothing of the shaders is restated there.  What WGSL and wgpu leave open is fixed as DESIGN.md §10 rules 2 and 3 fix it (the module's
header, R1-R4), the 8-bit image is encoded from the sRGB definition in binary64.  So:

  * every stage of post_ref.py - bloom_down, bloom_up, mix, hdr, fxaa, and post_ref's RGBA8 bytes - must reproduce EVERY WORD of every
    stored target of every case: executed-pipeline sky images, six seeded synthetic frames from 32 x 32 up (odd levels, a 1 x 1 level, HDR
    peaks, denormals, negative channels, alpha 0 / 0.25 / -1, edges into every border) and the eight uniform rows of test_post_uniforms;
  * the stored hit counts show that the fixture ran every statement, both outcomes of every condition and of every scalar select;
  * where the reference is present, fragments are re-executed from the shader text and must equal the committed arrays, and four
    mutations of the text (in memory) must each change stored bytes - the pin has teeth.

tests/test_gpu_display_pin.py holds the kernels to the same file; the kernels are held to post_ref.py by tests/test_gpu_display.py.
"""
import os
import re
import struct

import numpy as np
import pytest

import bhusie_amd as B
from oracle import wgsl_exec_post as WP
from tests import post_ref as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FROM_RAY_FIXTURE = ["rk_ladder", "rk_outside"]                 # their sky images are wgsl_exec.npz's `.sky` arrays
EXECUTED = ["mesh47", "direct45"]
SYNTH = ["s32x32", "s33x32", "s32x47", "s63x35", "s96x54", "s131x70"]
VARIANTS = ["low", "extreme", "it1", "it2", "it6", "it20", "mix0", "mix1"]
CASES = FROM_RAY_FIXTURE + EXECUTED + SYNTH + [f"s96x54.{v}" for v in VARIANTS]
HAVE_REF = WP.available()
needs_reference = pytest.mark.skipif(not HAVE_REF, reason="the reference's shaders are not on this machine")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "wgsl_exec_post.npz"))


@pytest.fixture(scope="module")
def ray_fixture():
    return np.load(os.path.join(GOLD, "wgsl_exec.npz"))


def sky_of(g, ray_fixture, name):
    if name in FROM_RAY_FIXTURE:
        return ray_fixture[f"{name}.sky"].view(np.float16)
    return g[f"{name.split('.')[0]}.sky"].view(np.float16)


def stored(g, name, key):
    """a target of a case; the uniform rows share s96x54's bloom levels, and its mix / hdr where no uniform reaches them"""
    if f"{name}.{key}" in g.files:
        return g[f"{name}.{key}"]
    base, _, variant = name.partition(".")
    if variant and (key.startswith("level") or variant not in ("mix0", "mix1")):
        return g[f"{base}.{key}"]
    return None


def uniforms_of(g, name):
    fb, mb = g[f"{name}.fxaa_details"].tobytes(), g[f"{name}.mix_details"].tobytes()
    e0, e1, it, sq = struct.unpack("<ffif", fb)
    return fb, mb, (np.float32(e0), np.float32(e1), it, np.float32(sq)), np.float32(struct.unpack("<f", mb)[0])


def _first(bad):
    return np.argwhere(bad)[:5].tolist()


def test_fixture_holds_the_cases_the_sizes_and_only_finite_data(g, ray_fixture):
    names = sorted({k.rsplit(".", 1)[0] for k in g.files if k.endswith(".rgba8")})
    assert names == sorted(CASES)
    sizes = {n: sky_of(g, ray_fixture, n).shape[:2] for n in CASES}
    assert [sizes[n][::-1] for n in SYNTH] == [(32, 32), (33, 32), (32, 47), (63, 35), (96, 54), (131, 70)]
    assert sizes["mesh47"] == (33, 47) and min(min(s) for s in sizes.values()) >= 32
    for n in CASES:
        sky = sky_of(g, ray_fixture, n).astype(np.float32)
        assert np.isfinite(sky).all() and np.isfinite(g[f"{n}.fxaa"]).all()
        assert g[f"{n}.fxaa"].shape == sky.shape and g[f"{n}.rgba8"].shape == sky.shape and g[f"{n}.rgba8"].dtype == np.uint8
    for n in SYNTH:                                                            # the content the issue lists, in every synthetic frame
        s = sky_of(g, ray_fixture, n)
        c = s[..., :3]
        for border, inner in ((c[0], c[1]), (c[-1], c[-2]), (c[:, 0], c[:, 1]), (c[:, -1], c[:, -2])):
            assert (border != inner).any(), f"{n}: no edge along a border"                        # the step across it leaves the frame: ClampToEdge
            assert (border[1:] != border[:-1]).any(), f"{n}: no edge running into a border"      # the search along it leaves the frame
        a = s[..., 3].astype(np.float32)
        assert {0.0, 0.25, -1.0, 1.0} <= set(np.unique(a)) and (s[..., :3] < 0).any() and (s[..., :3] == 0).any()
        sub = s[..., :3].view(np.uint16) & 0x7FFF
        assert ((sub > 0) & (sub < 0x0400)).any(), "binary16 denormals"
        assert int(g[f"{n}.seed"][0]) > 0
    peaks = sky_of(g, ray_fixture, "s63x35")[..., :3]
    assert float(peaks.max()) == 6.0e4 and (peaks == 6.0e4).sum() > 60 and float(g["s63x35.level0"].view(np.float16).max()) > 5.0e4
    for n in SYNTH:                                                            # the tone-mapped frames FXAA sees are pictures, not flat white
        if n != "s63x35":
            assert (g[f"{n}.hdr"].view(np.float16)[..., :3] < 0.5).mean() > 0.2, n
    # the direct leg's frame: only direction pixels and the horizon's constant
    f = g["direct45.frame"]
    hor = (f == np.array([0, 0, 0, 1], np.float32)).all(axis=-1)
    assert ((f[..., 3] == 0) | hor).all() and hor.any() and (f[..., 3] == 0).sum() > 500
    assert os.path.getsize(os.path.join(GOLD, "wgsl_exec_post.npz")) <= os.path.getsize(os.path.join(GOLD, "wgsl_exec.npz"))


def test_coverage_every_statement_condition_and_select_of_the_five_shaders_ran(g):
    for stage in WP.STAGES:
        c = {k: g[f"cov.{stage}.{k}"] for k in ("stmt_tok", "stmt_hits", "cond_tok", "cond_true", "cond_false", "sel_tok", "sel_true", "sel_false")}
        assert len(c["stmt_tok"]) >= 4 and len(c["stmt_tok"]) == len(c["stmt_hits"])
        assert (c["stmt_hits"] >= 1).all(), f"{stage}: statements at tokens {c['stmt_tok'][c['stmt_hits'] < 1].tolist()} never ran"
        assert (c["cond_true"] >= 1).all() and (c["cond_false"] >= 1).all(), f"{stage}: a condition came out one way only"
        assert (c["sel_true"] >= 1).all() and (c["sel_false"] >= 1).all(), f"{stage}: a select chose one way only"
    # fxaa: 10 ifs and the loop's condition (both arms of every `if`, the `break`, the bound reached), 9 scalar selects, 5 switch clauses
    assert len(g["cov.fxaa.cond_tok"]) >= 11 and len(g["cov.fxaa.sel_tok"]) >= 9 and len(g["cov.fxaa.stmt_tok"]) >= 90
    assert int(g["fxaa_past_early_exit"][0]) >= 1000


@pytest.mark.parametrize("name", CASES)
def test_post_ref_equals_the_executed_shaders_in_every_word(g, ray_fixture, name):
    sky16 = sky_of(g, ray_fixture, name)
    fb, mb, fx, mixr = uniforms_of(g, name)
    s = sky16.astype(np.float32)
    H, W = s.shape[:2]

    def same16(stage, got, want, channels=slice(None)):
        if want is None:
            return
        w = want.view(np.float16)[..., channels]
        got16 = np.asarray(got, np.float32).astype(np.float16)
        assert got16.shape == w.shape, f"{name}: {stage}: shape {got16.shape} != {w.shape}"
        bad = (got16.view(np.uint16) != w.view(np.uint16)).any(axis=-1)
        assert not bad.any(), f"{name}: first differing stage {stage}: {int(bad.sum())} pixels, first at (y, x) {_first(bad)}"

    img = s[..., :3]
    sizes = P.bloom_sizes(W, H)
    for i, (w, h) in enumerate(sizes):
        img = P.bloom_down(img, w, h) if i < 5 else P.bloom_up(img, w, h)
        want = stored(g, name, f"level{i}")
        same16(f"bloom level {i} ({w}x{h})", img, want, slice(0, 3))
        if want is not None:
            assert (want[..., 3] == 0x3C00).all(), f"{name}: bloom level {i}: alpha is not 1.0"
    mx = P.mix(s, img, mixr)
    same16("mix", mx, stored(g, name, "mix"))
    tone = P.hdr(mx)
    same16("hdr", tone, stored(g, name, "hdr"))
    fxaa = P.fxaa(tone, fx)
    want = g[f"{name}.fxaa"]
    bad = (fxaa.view(np.uint32) != want.view(np.uint32)).any(axis=-1)
    assert not bad.any(), f"{name}: first differing stage fxaa: {int(bad.sum())} pixels, first at (y, x) {_first(bad)}"
    got8 = P.post_ref(sky16, fx, mixr)
    bad = (got8 != g[f"{name}.rgba8"]).any(axis=-1)
    assert not bad.any(), f"{name}: first differing stage RGBA8 store: {int(bad.sum())} pixels, first at (y, x) {_first(bad)}"


def test_bloom_sizes_of_the_restatement_and_the_library_are_the_stored_level_shapes(g, ray_fixture):
    seen = 0
    for name in CASES:
        if f"{name}.level0" not in g.files:
            continue
        h, w = sky_of(g, ray_fixture, name).shape[:2]
        shapes = [g[f"{name}.level{i}"].shape for i in range(10)]
        assert [(s[1], s[0]) for s in shapes] == P.bloom_sizes(w, h) == B.bloom_sizes(w, h), name
        assert all(s[2] == 4 for s in shapes)
        seen += 1
    assert seen >= 7
    assert g["s32x32.level4"].shape[:2] == (1, 1) and g["s32x47.level1"].shape[:2] == (11, 8) and g["s63x35.level0"].shape[:2] == (17, 31)


def test_srgb_table_equals_the_binary64_definition_on_what_fxaa_produces_and_on_every_binary16(g):
    vals = np.unique(np.concatenate([g[f"{n}.fxaa"][..., :3].reshape(-1) for n in CASES]))
    assert vals.size > 20000
    assert np.array_equal(P.srgb_encode(vals), WP.srgb8(vals))
    half = np.arange(0x0000, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)       # all 31 744 non-negative finite binary16
    assert half.size == 31744 and np.array_equal(P.srgb_encode(half), WP.srgb8(half))
    # and where a table can go wrong: the f32 values on either side of every decision threshold.  (Until this pin the thresholds were rounded
    # to NEAREST f32; s96x54.it20 pixel (0, 12) holds 0.4764207 = the f32 below the real threshold of byte 184, which then took 184 for 183.)
    up = down = P.srgb_thresholds()
    near = [up]
    for _ in range(3):
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
        near += [up, down]
    near = np.unique(np.concatenate(near))
    assert near.size == 255 * 7 and np.array_equal(P.srgb_encode(near), WP.srgb8(near))
    assert WP.srgb8(np.float32(0.4764207)) == 183 == P.srgb_encode(np.float32(0.4764207))
    alpha = np.unique(np.concatenate([g[f"{n}.fxaa"][..., 3].reshape(-1) for n in CASES]))
    assert np.array_equal(P.unorm8(alpha), WP.unorm8(alpha))


# ---- only where the reference tree is present
@pytest.fixture(scope="module")
def pipeline():
    return WP.pipeline()


@needs_reference
@pytest.mark.parametrize("name", ["s33x32", "direct45"])
def test_fixture_is_what_executing_the_shader_text_gives(g, ray_fixture, pipeline, name):
    """64 seeded fragments of each of the 13 passes, re-executed from the files"""
    sky16 = sky_of(g, ray_fixture, name)
    fb, mb, _, _ = uniforms_of(g, name)
    levels = [g[f"{name}.level{i}"].view(np.float16) for i in range(10)]
    mix16, hdr16 = g[f"{name}.mix"].view(np.float16), g[f"{name}.hdr"].view(np.float16)
    rng = np.random.default_rng(64)
    targets = levels + [mix16, hdr16, g[f"{name}.fxaa"]]
    for k, want in enumerate(targets):
        h, w = want.shape[:2]
        n = min(64, w * h)
        pick = rng.choice(w * h, size=n, replace=False)
        px = [(int(p % w), int(p // w)) for p in pick]
        got = pipeline.run_stage(k, sky16, levels, mix16, hdr16, fb, mb, pixels=px)
        ref = np.stack([want[y, x] for x, y in px])
        if k < 12:
            assert np.array_equal(WP.to16(got).view(np.uint16), ref.view(np.uint16)), f"{name}: pass {k}"
        else:
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{name}: fxaa"
            enc = WP.encode_rgba8(got)
            assert np.array_equal(enc, np.stack([g[f"{name}.rgba8"][y, x] for x, y in px]))


def _mutate(stage, text):
    lines = text.split("\n")
    if stage == "fxaa132":                                                     # the sign at fxaa.wgsl:132
        assert "select(" in lines[131] and "reached2" in lines[131] and lines[131].count(" - ") == 1
        lines[131] = lines[131].replace(" - ", " + ")
        return "\n".join(lines)
    if stage == "quality5":
        out, n = re.subn(r"(case\s+5\s*:\s*\{\s*return\s+)[0-9.]+", r"\g<1>1.25", text)
    elif stage == "aces_m1":                                                   # the first two rows of the text of m1 exchanged
        m = re.search(r"m1\s*=\s*mat3x3\(\s*((?:-?[0-9.]+\s*,\s*){9})", text)
        nums = [v.strip() for v in m.group(1).split(",") if v.strip()]
        nums = nums[3:6] + nums[0:3] + nums[6:9]
        out, n = text[:m.start(1)] + ", ".join(nums) + ", " + text[m.end(1):], 1
    else:                                                                      # mix_ratio <-> 1.0 - mix_ratio
        out, n = re.subn(r"\(\s*1\.0\s*-\s*details\.mix_ratio\s*\)", "(@@)", text)
        out = out.replace("(details.mix_ratio)", "(1.0 - details.mix_ratio)").replace("(@@)", "(details.mix_ratio)")
    assert n == 1 and out != text
    return out


@needs_reference
@pytest.mark.parametrize("mutation,stage,case", [("fxaa132", "fxaa", "s32x32"), ("quality5", "fxaa", "s32x32"), ("aces_m1", "hdr", "s33x32"),
                                                 ("mix_swap", "mix", "s33x32")])
def test_the_pin_has_teeth(g, ray_fixture, mutation, stage, case):
    """A mutated copy of the text, in memory, changes stored bytes; the unmutated stage reproduces them (so the change is the mutation's)."""
    sky16 = sky_of(g, ray_fixture, case)
    fb, mb, _, _ = uniforms_of(g, case)
    levels = [g[f"{case}.level{i}"].view(np.float16) for i in range(10)]
    mix16, hdr16 = g[f"{case}.mix"].view(np.float16), g[f"{case}.hdr"].view(np.float16)
    k = {"mix": 10, "hdr": 11, "fxaa": 12}[stage]
    want = {"mix": mix16, "hdr": hdr16, "fxaa": g[f"{case}.fxaa"]}[stage]
    mutated = WP.Pipeline(sources={stage: _mutate(mutation, WP.shader_text(stage))})
    got = mutated.run_stage(k, sky16, levels, mix16, hdr16, fb, mb)
    if stage == "fxaa":
        changed = (WP.encode_rgba8(got) != g[f"{case}.rgba8"]).any(axis=-1)
        assert changed.sum() >= 1, f"{mutation}: no byte of the RGBA8 image changed"
    else:
        changed = (WP.to16(got).view(np.uint16) != want.view(np.uint16)).any(axis=-1)
        assert changed.sum() >= 1, f"{mutation}: no word of the {stage} target changed"
