"""CPU: the denoised stills (bhray_accum_read_denoised) without a device: bhray_accum_denoise_host - host arithmetic through the functions the kernels
call - held to the NumPy restatement (tests/accum_denoise_ref.py) in every word on seeded synthetic images; what the rule promises (the plain B3 a-trous under huge
sigmas, no bleeding over a coverage step, invalid pixels bit for bit); the refusals of the host form; the surface in the header, the library and the bindings."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import layouts
from tests import accum_denoise_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
E_INVALID = -1
FLT_MAX = float(np.finfo(np.float32).max)
SIZES = ((1, 1), (5, 3), (33, 32), (70, 37))                      # (w, h)
SUBSETS = [sum(c) for n in range(1, 5) for c in itertools.combinations(DR.PASSES, n)]
NAMES = {"bhray_accum_read_denoised": 4, "bhray_accum_read_display_denoised": 4, "bhray_accum_denoise_host": 6}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _params(iterations=3, guides=0, **sig):
    p = {"iterations": iterations, "guides": guides, "sigma_colour": 0.4, "sigma_coverage": 0.6, "sigma_closest": 1.5, "sigma_position": 3.0, "sigma_escape": 0.7}
    p.update(sig)
    return p


def _denoise(p):
    return B.StillDenoise(**p)


def synthetic(w, h, seed):
    """A colour mean and four guide means with everything the rule has a branch for: two regions with a coverage edge, alpha-0 pixels, NaN and Inf colour texels,
    non-finite guide values, a negative colour, a huge one, and (from 5 x 3 up) a valid pixel whose every tap - itself included - weighs 0."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    left = (xx + (yy // 3)) < (w // 2)
    c = np.empty((h, w, 4), F)
    c[..., 0:3] = np.where(left[..., None], 0.2, 1.5) + rng.uniform(0.0, 0.6, (h, w, 3))
    c[..., 3] = 1.0
    cov = np.zeros((h, w, 4), F)
    cov[..., 0] = np.where(left, 1.0, 0.0) * rng.uniform(0.8, 1.0, (h, w))
    cov[..., 1] = np.where(left, 0.0, 1.0) * rng.uniform(0.8, 1.0, (h, w))
    cov[..., 3] = 1.0
    geo = np.zeros((h, w, 4), F)
    geo[..., 0] = np.where(left, 2.0, 6.0) + rng.uniform(0.0, 1.0, (h, w))
    geo[..., 1] = rng.integers(3, 200, (h, w))
    geo[..., 2] = rng.uniform(0.0, 1.0, (h, w))
    geo[..., 3] = 1.0
    pos = np.zeros((h, w, 4), F)
    pos[..., 0:3] = np.where(left[..., None], 0.0, 1.0) * rng.uniform(-6.0, 6.0, (h, w, 3))
    pos[..., 3] = 1.0
    esc = np.zeros((h, w, 4), F)
    esc[..., 0:3] = rng.normal(0.0, 0.4, (h, w, 3))
    esc[..., 3] = 1.0
    n = w * h
    flat = lambda a: a.reshape(n, 4)
    pick = rng.permutation(n)
    k = max(1, n // 16) if n > 1 else 0
    for j, i in enumerate(pick[:k]):                              # pixels that are not valid, each in its own way
        kind = j % 4
        if kind == 0:
            flat(c)[i] = 0.0                                      # took no sample: zeros, alpha 0
            for g in (cov, geo, pos, esc):
                flat(g)[i] = 0.0
        elif kind == 1:
            flat(c)[i, j % 3] = np.nan
        elif kind == 2:
            flat(c)[i, (j + 1) % 3] = np.inf if j % 8 < 4 else -np.inf
        else:
            flat(c)[i, 3] = 0.5                                   # an alpha that is neither 0 nor 1 (the host form takes any image)
    for j, i in enumerate(pick[k:2 * k]):                         # valid pixels with guide values that are not finite: every tap from and to them weighs 0
        g = (cov, geo, pos, esc)[j % 4]
        flat(g)[i, 0] = (np.nan, np.inf, -np.inf)[j % 3]
    for i in pick[2 * k:2 * k + max(1, k // 2)] if n > 1 else ():
        flat(c)[i, 0:3] = (-0.5, 0.25, -0.125)                    # a negative luminance clamps to 0
    if n >= 15:
        flat(c)[pick[-1], 0:3] = (3.0e38, 3.0e38, 1.0e30)         # Y overflows: t = 1
        lonely = pick[-2]                                         # a valid pixel all of whose taps are invalid or weigh 0: NaN in EVERY guide, so whatever the subset
        for g in (cov, geo, pos, esc):
            flat(g)[lonely, 0:3] = np.nan
    return c, {DR.COVERAGE: cov, DR.GEOMETRY: geo, DR.POSITION: pos, DR.ESCAPE: esc}


def _same(got, want, what):
    bad = np.argwhere((_bits(got) != _bits(want)).any(axis=-1))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} pixels differ, first (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("iterations", (1, 2, 3, 4, 5))
def test_host_equals_the_restatement_at_every_iteration_count(w, h, iterations):
    c, g = synthetic(w, h, 100 * w + iterations)
    p = _params(iterations)
    got = B.accum_denoise_host(c, g, _denoise(p))
    _same(got, DR.denoise(c, g, p), f"{w}x{h}, {iterations} iterations")
    bad = ~DR.valid(c)
    assert np.array_equal(_bits(got)[bad], _bits(c)[bad]), "a pixel that is not valid comes back bit for bit"


@pytest.mark.parametrize("subset", SUBSETS)
def test_host_equals_the_restatement_for_every_guide_subset(subset):
    w, h = 33, 32
    c, g = synthetic(w, h, 7000 + subset)
    p = _params(5, guides=subset)                                 # spacing 16 reaches past the frame
    _same(B.accum_denoise_host(c, g, _denoise(p)), DR.denoise(c, g, p), f"guides 0x{subset:x} of the whole set")
    only = {b: g[b] for b in DR.PASSES if subset & b}
    p0 = _params(5, guides=0)
    _same(B.accum_denoise_host(c, only, _denoise(p0)), DR.denoise(c, only, p0), f"the planes 0x{subset:x} alone, guides 0")
    _same(B.accum_denoise_host(c, only, _denoise(p0)), B.accum_denoise_host(c, g, _denoise(p)), "guides 0 is the whole set")


def test_a_pixel_whose_taps_all_weigh_nothing_keeps_its_value():
    w, h = 9, 7
    c, g = synthetic(w, h, 5)
    c[...] = 0.0                                                  # every pixel but the centre took no sample
    c[3, 4] = (0.3, 0.6, 0.9, 1.0)
    p = _params(5)
    got = B.accum_denoise_host(c, g, _denoise(p))
    _same(got, DR.denoise(c, g, p), "one valid pixel among invalid ones")
    assert np.allclose(got[3, 4], c[3, 4], rtol=3e-7, atol=0.0), "its own tap is its only one: (w * c) / w per iteration"
    assert not _bits(got)[c[..., 3] == 0].any(), "the pixels that took no sample come back as the zeros they were"
    c2, g2 = synthetic(w, h, 6)
    c2[..., 0:3] = np.abs(c2[..., 0:3])
    c2[..., 3] = 1.0
    for plane in g2.values():
        plane[3, 4, 0:3] = np.nan                                 # valid, but every E of its own tap is E(NaN) = 0: ws = 0
    got2 = B.accum_denoise_host(c2, g2, _denoise(p))
    assert np.array_equal(_bits(got2[3, 4]), _bits(c2[3, 4]))
    _same(got2, DR.denoise(c2, g2, p), "ws == 0")


def _plain_b3(c, iterations):
    """the plain B3 a-trous of the valid pixels, in float64: weights h[|a|] h[|b|] over valid taps inside the frame, normalised"""
    cur = c.astype(np.float64)
    ok = DR.valid(c)
    h, w = ok.shape
    hh = (0.375, 0.25, 0.0625)
    for it in range(iterations):
        step = 1 << it
        acc, ws = np.zeros((h, w, 3)), np.zeros((h, w))
        for b in range(-2, 3):
            for a in range(-2, 3):
                q_ok = DR._shift(ok, a * step, b * step, False)
                cq = DR._shift(np.where(ok[..., None], cur[..., 0:3], 0.0), a * step, b * step, 0.0)
                wt = hh[abs(a)] * hh[abs(b)] * q_ok
                acc += wt[..., None] * cq
                ws += wt
        cur = cur.copy()
        cur[..., 0:3] = np.where(ok[..., None], acc / np.where(ws > 0, ws, 1.0)[..., None], cur[..., 0:3])
    return cur


@pytest.mark.parametrize("w,h", ((33, 32), (70, 37)))
def test_huge_sigmas_give_the_plain_b3_atrous(w, h):
    rng = np.random.default_rng(w)
    c, g = synthetic(w, h, 31)
    c[..., 0:3] = rng.uniform(0.0, 2.0, (h, w, 3))                # finite everywhere (an Inf guide difference over an Inf s2 is a NaN: weight 0)
    c[..., 3] = 1.0
    c[5, 6] = 0.0
    c[h - 1, w - 1, 1] = np.nan
    for plane in g.values():
        np.nan_to_num(plane, copy=False, nan=0.0, posinf=1.0, neginf=-1.0)
    p = _params(4, sigma_colour=FLT_MAX, sigma_coverage=FLT_MAX, sigma_closest=FLT_MAX, sigma_position=FLT_MAX, sigma_escape=FLT_MAX)
    got = B.accum_denoise_host(c, g, _denoise(p))
    _same(got, DR.denoise(c, g, p), "every sigma FLT_MAX")
    want = _plain_b3(c, 4)
    ok = DR.valid(c)
    assert np.allclose(got[ok][:, 0:3], want[ok][:, 0:3], rtol=2e-5, atol=0.0), "25 binary32 adds and a division per iteration against float64"
    assert np.array_equal(_bits(got)[~ok], _bits(c)[~ok])


def test_a_colour_step_at_a_coverage_step_does_not_bleed():
    w, h = 40, 24
    rng = np.random.default_rng(3)
    left = np.broadcast_to(np.arange(w) < 17, (h, w))
    c = np.ones((h, w, 4), F)
    c[..., 0:3] = np.where(left[..., None], rng.uniform(0.1, 0.3, (h, w, 3)), rng.uniform(2.0, 3.0, (h, w, 3)))
    cov = np.zeros((h, w, 4), F)
    cov[..., 0] = left                                            # horizon on the left, disk on the right: the coverage vectors are sqrt(2) apart
    cov[..., 1] = ~left
    cov[..., 3] = 1.0
    p = _params(5, sigma_colour=FLT_MAX, sigma_coverage=1.0)      # sigma_coverage below the step: E = 0 across it, whatever the colour term says
    got = B.accum_denoise_host(c, {DR.COVERAGE: cov}, _denoise(p))
    _same(got, DR.denoise(c, {DR.COVERAGE: cov}, p), "the step image")
    for side in (left, ~left):
        lo, hi = c[side][:, 0:3].min(), c[side][:, 0:3].max()
        eps = 1e-5 * hi                                           # the normalised sum of 25 rounded terms may leave the range by roundings only
        assert got[side][:, 0:3].min() >= lo - eps and got[side][:, 0:3].max() <= hi + eps, "each side's outputs lie within that side's input range"
    assert np.abs(got[left][:, 0:3] - c[left][:, 0:3]).max() > 1e-3, "and the filter did smooth"


def test_parameter_refusals_of_the_host_form():
    L = B.lib()
    w, h = 5, 3
    c, g = synthetic(w, h, 1)
    out = np.full_like(c, 7.0)
    planes = (C.c_void_p * 4)(*[g[b].ctypes.data for b in DR.PASSES])

    def call(st, planes=planes, colour=c, ww=w, hh=h, dst=out):
        return L.bhray_accum_denoise_host(colour.ctypes.data if colour is not None else None, planes, ww, hh, C.byref(st) if st is not None else None,
                                          dst.ctypes.data if dst is not None else None)

    d = layouts.BhrayStillDenoise()
    L.bhray_still_denoise_default(C.byref(d))
    assert d.struct_size == C.sizeof(layouts.BhrayStillDenoise) == 32 and 1 <= d.iterations <= 5 and d.guides == 0
    assert all(np.isfinite(getattr(d, f)) and getattr(d, f) > 0 for f in ("sigma_colour", "sigma_coverage", "sigma_closest", "sigma_position", "sigma_escape"))
    L.bhray_still_denoise_default(None)                           # a NULL is ignored
    assert call(d) == 0 and call(None) == 0
    assert np.array_equal(_bits(out), _bits(B.accum_denoise_host(c, g))), "NULL parameters are the defaults"

    def bad(**kw):
        s = layouts.BhrayStillDenoise()
        L.bhray_still_denoise_default(C.byref(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    out[...] = 7.0
    for s in (bad(struct_size=28), bad(struct_size=0), bad(iterations=0), bad(iterations=6), bad(guides=0x10), bad(guides=0x1F),
              bad(sigma_colour=0.0), bad(sigma_coverage=-1.0), bad(sigma_closest=float("nan")), bad(sigma_position=float("inf")), bad(sigma_escape=-0.0)):
        assert call(s) == E_INVALID
    two = (C.c_void_p * 4)(g[1].ctypes.data, None, g[4].ctypes.data, None)
    assert call(bad(guides=2), planes=two) == E_INVALID, "a guide whose plane is absent"
    assert call(bad(guides=5), planes=two) == 0
    out[...] = 7.0
    assert call(d, planes=(C.c_void_p * 4)()) == E_INVALID, "no plane present: the filter has no guide"
    assert call(d, planes=None) == E_INVALID and call(d, colour=None) == E_INVALID and call(d, dst=None) == E_INVALID
    assert call(d, ww=0) == E_INVALID and call(d, hh=0) == E_INVALID
    assert (out == 7.0).all(), "a refused call writes nothing"
    with pytest.raises(B.BhrayError):
        B.accum_denoise_host(c, g, B.StillDenoise(iterations=9))


def test_the_surface():
    L = B.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bhray.h")).read(), flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, f"{name} is not declared in bhray.h"
        assert m.group(1).count(",") + 1 == nargs == len(layouts.SYMBOLS[name][1]), name
        assert layouts.SYMBOLS[name][0] is C.c_int and name not in layouts.DIAG_SYMBOLS
        assert len(getattr(L, name).argtypes) == nargs           # AttributeError: not exported
    assert re.search(r"\bvoid\s+bhray_still_denoise_default\s*\(", hdr) and "bhray_still_denoise_default" in layouts.SYMBOLS
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert L.bhray_version() & 0xFFFF == 5
    assert re.search(r"#define BHRAY_DENOISE_MAX_ITERATIONS 5u", hdr) and layouts.DENOISE_MAX_ITERATIONS == 5
    for name in ("accum_read_denoised", "accum_read_display_denoised"):
        assert callable(getattr(B.RayPass, name))
    d = B.StillDenoise()
    assert (d.iterations, d.guides) == (B.StillDenoise(iterations=None).iterations, 0) and d.struct().struct_size == 32
    assert B.StillDenoise(iterations=2, sigma_escape=0.25).struct().sigma_escape == 0.25
