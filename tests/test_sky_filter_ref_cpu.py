"""CPU: the NumPy restatement of the footprint-filtered sky pass (tests/sky_filter_ref.py) - that it is np_ray.sky_resolve when nothing is
filtered, its pyramid sizes, its level rule, that a constant sky stays constant, that the filter lowers the error against a supersampled truth, and that the
coverage floors tests/test_gpu_sky_filter.py asks of the device's frame hold on np_ray's frame of the same scene."""
import functools

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from oracle import np_ray as N
from tests import common as T
from tests import sky_filter_ref as S

W, H = 64, 36

@functools.lru_cache(maxsize=None)
def frame(method=1, size=(W, H)):
    u = T.uniforms(integration_method=method)
    return N.render_level(N.Scene(*u, *T.textures()), size)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def test_unfiltered_is_np_rays_sky_resolve_bit_for_bit():
    sky = T.textures()[2]
    f = frame().copy()
    f[3, 5] = (np.nan, 0.5, 0.5, 0.0); f[4, 7] = (0.0, 0.0, 0.0, 0.0); f[5, 9] = (-0.0, 1.0, -0.0, 0.0); f[6, 11] = (np.inf, 1.0, 0.0, 0.0)
    f[7, 13] = (0.1, 0.2, 0.3, np.nan)
    got, st = S.resolve(f, sky, enabled=False)
    with np.errstate(invalid="ignore"):
        want = N.sky_resolve(f, sky)
    assert np.array_equal(_bits(got), _bits(want))
    assert st["filtered"] == 0 and st["direction"] > 1900


@pytest.mark.parametrize("w,h,want", [
    (5, 3, [(5, 3), (3, 2), (2, 1), (1, 1)]),
    (1, 7, [(1, 7), (1, 4), (1, 2), (1, 1)]),
    (512, 256, [(512 >> l, max(256 >> l, 1)) for l in range(10)]),
])
def test_pyramid_sizes(w, h, want):
    assert S.sizes(w, h) == want
    rng = np.random.default_rng(w * 100 + h)
    pyr = S.pyramid(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))
    assert [(p.shape[1], p.shape[0]) for p in pyr] == want
    assert all(p.dtype == np.float16 and (p[..., 3] == 1.0).all() for p in pyr[1:])


def test_odd_level_clamps_its_last_block():
    t = np.zeros((3, 5, 4), np.uint8)
    t[..., 0] = 255
    t[2, 4, 0] = 0                                              # the corner texel: its block is that texel four times
    pyr = S.pyramid(t)
    assert pyr[1][1, 2, 0] == 0.0 and pyr[1][0, 0, 0] == 1.0 and pyr[1][1, 0, 0] == 1.0


def test_exponent_and_fraction_rule():
    L, f = S.level_and_fraction(np.array([1.0, 1.5, 2.0, 3.999], np.float32))
    assert L.tolist() == [0, 0, 1, 1]
    assert f[0] == 0.0 and f[1] == 0.5 and f[2] == 0.0
    assert f[3] == np.float32(np.float32(3.999) * np.float32(0.5)) - np.float32(1.0) and 0.999 < f[3] < 1.0


def test_constant_sky_stays_constant_at_every_level():
    sky = np.full((150, 301, 4), 200, np.uint8)
    pyr = S.pyramid(sky)
    c = np.float32(200) / np.float32(255)
    c4 = np.float16((c * c) * (c * c))
    for lvl in pyr[1:]:
        assert (lvl[..., 0:3] == c4).all()
    got, st = S.resolve(frame(), sky, pyr)
    plain, _ = S.resolve(frame(), sky, pyr, enabled=False)
    assert st["filtered"] > 500 and len(st["levels"]) >= 2
    m = st["mask"]
    # level 0 gives c^4 in binary32, the levels above its binary16 rounding: every blend and every mean of the two rounds to that binary16 value
    assert (got[m][:, 0:3] == c4).all() and (got[m][:, 3] == 1.0).all()
    assert np.array_equal(_bits(got[~m]), _bits(plain[~m]))


def test_the_filter_lowers_the_error_against_a_supersampled_truth():
    sky = T.textures()[2]
    small = frame()
    big = frame(size=((W - 1) * 4 + 1, (H - 1) * 4 + 1))
    assert np.array_equal(big[::4, ::4].view(np.uint32), small.view(np.uint32)), "the large frame's grid contains the small frame's"
    with np.errstate(invalid="ignore"):
        res = N.sky_resolve(big, sky).astype(np.float64)[..., 0:3]
    hb, wb = res.shape[:2]
    truth = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            y0, y1 = max(4 * y - 2, 0), min(4 * y + 2, hb - 1) + 1
            x0, x1 = max(4 * x - 2, 0), min(4 * x + 2, wb - 1) + 1
            truth[y, x] = res[y0:y1, x0:x1].reshape(-1, 3).mean(axis=0)
    filt, st = S.resolve(small, sky)
    plain, _ = S.resolve(small, sky, enabled=False)
    d = small[..., 3] == 0
    rms = lambda img: float(np.sqrt(((img[..., 0:3].astype(np.float64) - truth)[d] ** 2).mean()))
    e_f, e_p = rms(filt), rms(plain)
    print(f"rms filtered {e_f:.5f} unfiltered {e_p:.5f} over {int(d.sum())} direction pixels")
    assert e_f < e_p, (e_f, e_p)


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_gpu_tests_coverage_floors_hold_on_np_rays_frame(method):
    sky = T.textures()[2]
    got, st = S.resolve(frame(method), sky)
    plain, _ = S.resolve(frame(method), sky, enabled=False)
    print({k: v for k, v in st.items() if k != "mask"})
    S.check_floors(st)
    assert int((_bits(got) != _bits(plain)).any(axis=-1).sum()) >= 1000


def test_deep_and_magnified_floors_hold_on_np_rays_frame():
    big = assets.sky_texture(4096, 2048, seed=2)
    _, st = S.resolve(frame(), big)
    print({k: v for k, v in st.items() if k != "mask"})
    assert st["taps"][8] >= 25 and all(st["levels"].get(l, 0) > 0 for l in range(2, 7)), st
    tiny = assets.sky_texture(64, 32, seed=2)
    _, st = S.resolve(frame(), tiny)
    print({k: v for k, v in st.items() if k != "mask"})
    assert st["direction"] - st["filtered"] >= 1500 and st["filtered"] >= 1
