"""CPU: the arithmetic claims behind the phases' short sequences (bhray_kernels.hip, BHRAY_PHASE_SEQ) that need no device.

unorm8_rn - a texel's byte as unorm, x * RN(1/255) with one fused residual correction - must be the correctly rounded x / 255 for every byte; two_over_rn relies on
2 * RN(1/x) == RN(2/x) inside rcp_rn's range; dist_rsqrt_rn and normalize_ph put ONE range test in front of a root followed by a root and/or a reciprocal, which needs the
root of an in-range radicand to lie inside the later sequences' ranges.  The sequences themselves (v_rcp_f32 / v_rsq_f32 and their corrections) are checked on the
device, against the IEEE forms, by bhray_selftest."""
import re
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rn32(q: Fraction) -> np.float32:
    """q rounded to the nearest binary32, ties to even, in exact arithmetic (normal results only)"""
    if q == 0:
        return np.float32(0.0)
    c = np.float32(float(q))                     # within one ulp of the answer: pick among the neighbours exactly
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(v.view(np.uint32)) & 1))


def fma32(a, b, c) -> np.float32:
    return rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_unorm8_rn_is_the_correctly_rounded_quotient_for_every_byte():
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_kernels.hip")).read()
    m = re.search(r"float unorm8_rn\(float x\) \{\s*const float r = (\S+)f;", src)
    assert m, "unorm8_rn's constant not found"
    r = np.float32(float.fromhex(m.group(1)))
    assert r == rn32(Fraction(1, 255)), "the constant is RN(1/255)"
    plain_product_wrong = 0
    for x in range(256):
        want = rn32(Fraction(x, 255))
        q0 = rn32(Fraction(x) * Fraction(float(r)))
        got = fma32(fma32(np.float32(-255.0), q0, np.float32(x)), r, q0)
        assert got.view(np.uint32) == want.view(np.uint32), (x, got, want)
        assert want == np.float32(x) / np.float32(255.0)                 # and the host's IEEE division agrees with the exact rounding
        plain_product_wrong += int(q0.view(np.uint32) != want.view(np.uint32))
    assert plain_product_wrong > 0, "the residual correction is needed: the product alone is not the quotient"


def test_twice_the_rounded_reciprocal_is_the_rounded_quotient_of_two():
    """2 * RN(1/x) == RN(2/x) for 2^-125 <= x < 2^126 (rcp_in_range): seeded bit patterns over every exponent of the range, and its ends"""
    rng = np.random.default_rng(15)
    exps = np.repeat(np.arange(2, 253, dtype=np.uint32), 4096)          # biased exponents 2 .. 252: 2^-125 .. below 2^126
    bits = (exps << np.uint32(23)) | rng.integers(0, 1 << 23, size=exps.size, dtype=np.uint32)
    bits = np.concatenate([bits, np.array([0x01000000, 0x01000001, 0x7e7fffff, 0x3f800000, 0x3f7fffff], dtype=np.uint32)])
    x = bits.view(np.float32)
    assert ((bits - np.uint32(0x01000000)) < np.uint32(0x7d800000)).all()
    a = np.float32(2.0) * (np.float32(1.0) / x)
    b = np.float32(2.0) / x
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(a).all() and (np.abs(a) >= np.float32(2.0 ** -125)).all()


def test_one_range_test_covers_the_sequences_behind_a_root():
    """sqrt_in_range is [2^-95, 2^95]; rcp_in_range [2^-125, 2^126): the root of an in-range radicand, and that root's root, lie inside both"""
    lo, hi = np.float32(2.0 ** -95), np.float32(2.0 ** 95)
    for d2 in (lo, hi):
        dist = np.sqrt(d2)
        root = np.sqrt(dist)
        for v in (dist, root):
            assert lo <= v <= hi
            assert np.float32(2.0 ** -125) <= v < np.float32(2.0 ** 126)
