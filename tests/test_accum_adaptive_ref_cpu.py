"""CPU: the restatement of adaptive stills (tests/accum_adaptive_ref.py) on synthetic sample streams with known answers - the yardstick of
tests/test_gpu_accum_adaptive.py must itself be right."""
import numpy as np
import pytest

import bhusie_amd as B
from tests import accum_adaptive_ref as R
from tests import accum_ref as A
from tests import common as T
from tests import rays_ref as RR

F = np.float32


def _stream(pixels, S):
    """results[s] (npix, 4) from per-pixel functions s -> (r, g, b); alpha 1, so the resolve passes them through"""
    out = np.ones((S, len(pixels), 4), F)
    for p, f in enumerate(pixels):
        for s in range(S):
            out[s, p, 0:3] = f(s)
    return out


CONST = lambda s: (0.25, 0.5, 0.125)
ALT = lambda s: (float(s & 1),) * 3
NAN = lambda s: (np.nan, 0.0, 0.0)
NOISY = lambda s: (0.5 + 0.01 * ((s * 7) % 5), 0.5, 0.5)


def test_constant_alternating_and_nan_pixels():
    res = _stream([CONST, ALT, NAN], 16)
    st = R.State(3)
    info, actives = R.call(st, R.Params(4, 16, 4, 0.05, 0.01), res)
    assert st.issued.tolist() == [4, 16, 16], "a constant pixel stops at min_samples; 0/1 alternation and an all-NaN pixel go to max_samples"
    assert st.sum[:, 3].tolist() == [4.0, 16.0, 0.0]
    assert [a.tolist() for a in actives] == [[1, 2]] * 3
    assert info == {"rounds": 4, "active_last": 0, "rays": 3 * 4 + 3 * 2 * 4, "reach": 16}
    m = R.mean(st)
    assert np.array_equal(m[0], np.array([0.25, 0.5, 0.125, 1.0], F)) and np.array_equal(m[1], np.array([0.5, 0.5, 0.5, 1.0], F))
    assert not m[2].any() and st.S1[2] == 0 and st.S2[2] == 0, "n == 0: a mean of zeros"
    assert not R.converged(st, 1e30, 1.0)[2], "0 / 0 is a NaN and a comparison with a NaN is false"


def test_zero_tolerance_stops_exactly_the_zero_variance_pixels():
    # 0.25, 0.5, 0.125 and their luminance sums are exact in binary32 only by luck; a power-of-two grey is exact by construction: Y = 1, t = 0.5, S1 = n / 2, S2 = n / 4
    grey = lambda s: (1.0, 1.0, 1.0)
    black = lambda s: (0.0, 0.0, 0.0)
    res = _stream([grey, black, NOISY, ALT], 12)
    st = R.State(4)
    R.call(st, R.Params(4, 12, 4, 0.0, 0.0), res)
    # (0.2126 + 0.7152) + 0.0722 need not be 1 in binary32, but it is the same t every sample; whether q - m * m is then 0 is what the rule says, not what this test assumes:
    t = R.luminance_t(np.array([[1.0, 1.0, 1.0]], F))[0]
    n = F(4)
    s1 = F(F(F(t + t) + t) + t); s2 = F(F(F(F(t * t) + F(t * t)) + F(t * t)) + F(t * t))
    m = F(s1 / n); v = F(F(s2 / n) - F(m * m))
    assert st.issued[0] == (4 if v <= 0 else 12)
    assert st.issued[1] == 4, "black: S1 = S2 = 0, v = 0 <= 0"
    assert st.issued[2] == 12 and st.issued[3] == 12, "any variance fails a zero tolerance"


def test_one_call_equals_two_calls():
    pixels = [CONST, ALT, NOISY, NAN, lambda s: (0.0, 0.0, 0.0) if s < 9 else (4.0, 4.0, 4.0)]
    res = _stream(pixels, 16)
    one = R.State(5)
    i1, _ = R.call(one, R.Params(4, 16, 4, 0.02, 0.01), res)
    two = R.State(5)
    ia, _ = R.call(two, R.Params(4, 8, 4, 0.02, 0.01), res)
    assert two.issued.max() == 8
    ib, _ = R.call(two, R.Params(4, 16, 4, 0.02, 0.01), res)
    for a, b in ((one.sum, two.sum), (one.S1, two.S1), (one.S2, two.S2), (one.issued, two.issued)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ia["rays"] + ib["rays"] == i1["rays"] and ia["rounds"] + ib["rounds"] == i1["rounds"] and ib["reach"] == i1["reach"] == 16
    assert one.issued[4] == 4, "the known property: a pixel that looked quiet early has stopped before its stream changes"


def test_a_smaller_tolerance_continues():
    res = _stream([CONST, NOISY], 12)
    st = R.State(2)
    R.call(st, R.Params(4, 12, 4, 0.5, 0.01), res)
    assert st.issued.tolist() == [4, 4]
    info, actives = R.call(st, R.Params(4, 12, 4, 1e-4, 0.01), res)
    assert st.issued.tolist() == [4, 12] and info["rounds"] == 2 and info["rays"] == 8 and [a.tolist() for a in actives] == [[1], [1]]


def test_the_luminance_clamp_and_the_big_branch():
    t = R.luminance_t(np.array([[-1.0, -1.0, -1.0], [0.0, 0.0, 0.0], [1e38, 1e38, 1e38], [3e38, 3e38, 3e38], [2.0 ** 100, 2.0 ** 100, 2.0 ** 100], [1e30, 0, 0]], F))
    assert t[0] == 0 and t[1] == 0, "a negative luminance is clamped to 0"
    assert t[2] == 1 and t[4] == 1, "from 2^100 on t is 1 (Y / (1 + Y) would still round to 1 there, an infinite Y would give a NaN)"
    assert t[3] == 1, "a finite colour whose luminance overflows: inf >= 2^100"
    assert t[5] == F(F(F(0.2126) * F(1e30)) / F(F(1) + F(F(0.2126) * F(1e30)))) and t[5] <= 1
    y = F(3.0)
    one = R.luminance_t(np.array([[0.0, 0.0, y / F(0.0722)]], F))[0]
    Y = F(F(0.0722) * F(y / F(0.0722)))
    assert one == F(Y / F(F(1) + Y)) and abs(float(one) - 0.75) < 1e-6
    st = R.State(1)
    R.add_sample(st, np.array([0]), np.array([[np.inf, 0.0, 0.0, 1.0]], F))
    assert st.sum[0, 3] == 0 and st.S1[0] == 0, "a sample that is not finite is skipped"


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_gpu_tests_tolerance_splits_the_frame(method):
    """The parameters of tests/test_gpu_accum_adaptive.py (R.GPU_TEST), judged without a device: oracle.trace_ray over the sample rays of the 40 x 36 frame."""
    cam, cfg, tex = B.Camera(), B.ladder_for_frame((40, 36), 3, 2), T.textures()
    sc = T.oracle_scene(*T.uniforms(camera=cam, integration_method=method), tex)
    p = R.GPU_TEST
    assert (p.min_samples, p.round_samples, p.max_samples) == (4, 4, 12)
    res = [RR.oracle_rays(sc, A.sample_rays(cam, cfg, s))[0] for s in range(p.max_samples)]
    st = R.State(res[0].shape[0])
    R.call(st, p, res, tex[2])
    stop, more, top = float((st.issued == 4).mean()), float((st.issued > 4).mean()), int((st.issued == 12).sum())
    print(f"method {method}: {100 * stop:.1f} % stop at 4, {100 * more:.1f} % take more, {top} of {st.issued.size} reach 12")
    assert set(np.unique(st.issued).tolist()) <= {4, 8, 12}
    assert stop >= 0.10 and more >= 0.10 and top >= 1
