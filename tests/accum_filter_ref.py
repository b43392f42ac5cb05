"""The still pixel filters (bhray_accum_set_filter) restated in NumPy from include/bhray.h's contract, binary32 operation by operation: the ten weights
of a sample, the resolved result image V, the 5 x 5 double loop and the sum in sample order.  What tests/test_accum_filter_cpu.py and tests/test_gpu_accum_filter.py
compare with.  The offsets, the sky resolve and the mean are tests/accum_ref.py's."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import accum_ref as A

F = np.float32
BOX, TENT, CUBIC = 0, 1, 2


@dataclass(frozen=True)
class Filter:
    kind: int = BOX
    radius: float = 2.0
    b: float = 1.0 / 3.0
    c: float = 1.0 / 3.0


def tent(radius=1.0):
    return Filter(TENT, radius)


def cubic(radius=2.0, b=1.0 / 3.0, c=1.0 / 3.0):
    return Filter(CUBIC, radius, b, c)


def coefficients(b, c):
    """(p3, p2, p0), (q3, q2, q1, q0): formed in binary64 from the binary32 b and c, rounded once"""
    B, C = float(F(b)), float(F(c))
    p = (F((12.0 - 9.0 * B - 6.0 * C) / 6.0), F((-18.0 + 12.0 * B + 6.0 * C) / 6.0), F((6.0 - 2.0 * B) / 6.0))
    q = (F((-B - 6.0 * C) / 6.0), F((6.0 * B + 30.0 * C) / 6.0), F((-12.0 * B - 48.0 * C) / 6.0), F((8.0 * B + 24.0 * C) / 6.0))
    return p, q


def offsets(s):
    """tests/accum_ref.offset for an array of sample indices: (dx, dy), float32 arrays of s's shape (every step exact in binary32)"""
    s = np.asarray(s, dtype=np.uint64)
    u = (np.uint64(0x80000000) + s * np.uint64(0xC13FA9A9)) & np.uint64(0xFFFFFFFF)
    v = (np.uint64(0x80000000) + s * np.uint64(0x91E10DA5)) & np.uint64(0xFFFFFFFF)
    dx = ((u >> np.uint64(8)).astype(F) * F(2.0 ** -24)).astype(F) - F(0.5)
    dy = ((v >> np.uint64(8)).astype(F) * F(2.0 ** -24)).astype(F) - F(0.5)
    return dx.astype(F), dy.astype(F)


def k(filt: Filter, t) -> np.ndarray:
    """the filter at the distances t >= 0 (binary32, any shape), one rounded operation per step"""
    t = np.asarray(t, dtype=F)
    zero = np.zeros_like(t)
    if filt.kind == TENT:
        a = (t / F(filt.radius)).astype(F)
        return np.where(a < F(1.0), (F(1.0) - a).astype(F), zero).astype(F)
    inv = F(F(2.0) / F(filt.radius))
    x = (t * inv).astype(F)
    (p3, p2, p0), (q3, q2, q1, q0) = coefficients(filt.b, filt.c)
    near = ((((p3 * x).astype(F) + p2).astype(F) * (x * x).astype(F)).astype(F) + p0).astype(F)
    far = ((((((q3 * x).astype(F) + q2).astype(F) * x).astype(F) + q1).astype(F) * x).astype(F) + q0).astype(F)
    return np.where(x < F(1.0), near, np.where(x < F(2.0), far, zero)).astype(F)


def weights_table(filt: Filter, s, reach: int = 2):
    """(wx, wy) of the samples s (an array of n indices): float32 arrays (n, 2 * reach + 1) - tap i at float(i) + dx (dy)"""
    s = np.atleast_1d(np.asarray(s))
    taps = np.arange(-reach, reach + 1).astype(F)
    if filt.kind == BOX:
        w = np.zeros((s.size, 2 * reach + 1), F)
        w[:, reach] = 1.0
        return w, w.copy()
    dx, dy = offsets(s)
    wx = k(filt, np.abs((taps[None, :] + dx[:, None]).astype(F)))
    wy = k(filt, np.abs((taps[None, :] + dy[:, None]).astype(F)))
    return wx, wy


def weights(filt: Filter, s: int, reach: int = 2):
    """(wx, wy) of sample s, float32 arrays of 2 * reach + 1 taps.  reach = 2 is the contract; 3 shows that taps +-3 weigh nothing."""
    wx, wy = weights_table(filt, [int(s)], reach)
    return wx[0], wy[0]


def resolved_image(results, t_sky, w: int, h: int) -> np.ndarray:
    """V: (h, w, 4) - (r, g, b, 1) of the resolved result where r, g, b are finite, zeros elsewhere (a select)"""
    c = A.resolve(results, t_sky)
    ok = A.taken(c)
    v = np.zeros((h * w, 4), F)
    v[ok, 0:3] = c[ok, 0:3]
    v[ok, 3] = 1.0
    return v.reshape(h, w, 4)


def stencil(V, wx, wy) -> np.ndarray:
    """c(x, y) = sum_j wy[j] * (sum_i wx[i] * V(x + i, y + j)), both sums from zero in increasing tap order, V zero outside the frame; every step rounded to binary32"""
    h, w = V.shape[0:2]
    r = (len(wx) - 1) // 2
    pad = np.zeros((h + 2 * r, w + 2 * r, 4), F)
    pad[r:r + h, r:r + w] = V
    c = np.zeros((h, w, 4), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(2 * r + 1):
            row = np.zeros((h, w, 4), F)
            for i in range(2 * r + 1):
                row = (row + (F(wx[i]) * pad[j:j + h, i:i + w]).astype(F)).astype(F)
            c = (c + (F(wy[j]) * row).astype(F)).astype(F)
    return c


def accumulate(per_sample_results, t_sky, filt: Filter, w: int, h: int, s0: int = 0, reach: int = 2) -> np.ndarray:
    """the sum over samples s0, s0 + 1, ... in order: (h * w, 4) float32, .w = the weight received"""
    total = np.zeros((h, w, 4), F)
    for n, r in enumerate(per_sample_results):
        wx, wy = weights(filt, s0 + n, reach)
        with np.errstate(over="ignore", invalid="ignore"):
            total = (total + stencil(resolved_image(r, t_sky, w, h), wx, wy)).astype(F)
    return total.reshape(h * w, 4)


def kappa(per_sample_results, t_sky, filt: Filter, w: int, h: int, s0: int = 0) -> float:
    """max over pixels of sum |weight| / |sum weight| over every tap of every sample the pixel received (binary64 over the binary32 weights): 1 for a filter
    without negative lobes"""
    absw = np.zeros((h, w), np.float64)
    sumw = np.zeros((h, w), np.float64)
    for n, r in enumerate(per_sample_results):
        wx, wy = weights(filt, s0 + n)
        vw = np.zeros((h + 4, w + 4), np.float64)
        vw[2:2 + h, 2:2 + w] = resolved_image(r, t_sky, w, h)[..., 3]
        for j in range(5):
            for i in range(5):
                t = float(wx[i]) * float(wy[j]) * vw[j:j + h, i:i + w]
                sumw += t
                absw += np.abs(t)
    return float((absw / np.abs(sumw)).max())


def skipped_in_support(per_sample_results, t_sky, filt: Filter, w: int, h: int, s0: int = 0) -> np.ndarray:
    """(h, w) bool: the pixel has, in some sample, a skipped (not finite) texel inside the frame under a tap of non-zero weight"""
    out = np.zeros((h, w), bool)
    for n, r in enumerate(per_sample_results):
        wx, wy = weights(filt, s0 + n)
        miss = np.zeros((h + 4, w + 4), bool)
        miss[2:2 + h, 2:2 + w] = resolved_image(r, t_sky, w, h)[..., 3] == 0
        for j in range(5):
            for i in range(5):
                if wx[i] != 0 and wy[j] != 0:
                    out |= miss[j:j + h, i:i + w]
    return out
