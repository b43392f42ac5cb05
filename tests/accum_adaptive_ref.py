"""Adaptive stills (bhray_accum_add_adaptive) restated in NumPy, binary32 one operation at a time: a sample added to a pixel's sum and to the two moments
of its compressed luminance, the per-pixel test, and the rounds of a call.  The offsets, the sample rays and the resolve are tests/accum_ref.py's.  What
tests/test_accum_adaptive_ref_cpu.py and tests/test_gpu_accum_adaptive.py compare with."""
from __future__ import annotations

import numpy as np

from tests import accum_ref as A

F = np.float32
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)
BIG = F(2.0 ** 100)


class Params:
    def __init__(self, min_samples=4, max_samples=12, round_samples=4, tolerance=0.05, dark=0.01):
        self.min_samples, self.max_samples, self.round_samples = int(min_samples), int(max_samples), int(round_samples)
        self.tolerance, self.dark = F(tolerance), F(dark)

    def as_kwargs(self):
        return {"min_samples": self.min_samples, "max_samples": self.max_samples, "round_samples": self.round_samples,
                "tolerance": float(self.tolerance), "dark": float(self.dark)}


# What tests/test_gpu_accum_adaptive.py runs with.  Chosen on the CPU from oracle.trace_ray over samples 0 .. 11 of the 40 x 36 frame's rays (default scene, either
# integrator): under min 4 / round 4 / max 12 about 76 % of the pixels stop at 4, 24 % take more and 19 % reach 12 (tests/test_accum_adaptive_ref_cpu.py asserts
# at least 10 % / 10 % / one pixel; DESIGN.md §20 has the shares).
GPU_TEST = Params(4, 12, 4, 0.05, 0.01)


class State:
    """sum (n, 4), S1, S2 (n,) float32 and issued (n,) uint32: all zero after begin; mode: the (min_samples, round_samples) of the first call, or None"""

    def __init__(self, npix):
        self.sum = np.zeros((npix, 4), F)
        self.S1 = np.zeros(npix, F)
        self.S2 = np.zeros(npix, F)
        self.issued = np.zeros(npix, np.uint32)
        self.mode = None


def luminance_t(rgb) -> np.ndarray:
    """t of resolved colours (n, 3): Y = (0.2126 r + 0.7152 g) + 0.0722 b, clamped at 0, compressed Y / (1 + Y) (1 from 2^100 on)"""
    rgb = np.asarray(rgb, F)
    with np.errstate(over="ignore", invalid="ignore"):
        Y = ((KR * rgb[:, 0]) + (KG * rgb[:, 1])) + (KB * rgb[:, 2])
        Y = np.where(Y < 0, F(0), Y).astype(F)
        big = Y >= BIG
        t = np.where(big, F(1), Y / (F(1) + np.where(big, F(0), Y))).astype(F)
    assert t.dtype == F
    return t


def add_sample(st: State, pix, resolved):
    """pixels `pix` (indices) take the resolved colours (len(pix), 4): skipped where r, g or b is not finite"""
    pix = np.asarray(pix)
    ok = A.taken(resolved)
    p, c = pix[ok], resolved[ok]
    add = np.concatenate([c[:, 0:3], np.ones((c.shape[0], 1), F)], axis=1)
    st.sum[p] = (st.sum[p] + add).astype(F)
    t = luminance_t(c[:, 0:3])
    st.S1[p] = (st.S1[p] + t).astype(F)
    st.S2[p] = (st.S2[p] + (t * t).astype(F)).astype(F)


def converged(st: State, tolerance, dark) -> np.ndarray:
    """the test: n = sum.w, m = S1 / n, q = S2 / n, v = max(q - m * m, 0) (a NaN stays), e = tolerance * (m + dark); v <= (e * e) * n (false for a NaN)"""
    tol, dark = F(tolerance), F(dark)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = st.sum[:, 3]
        m = (st.S1 / n).astype(F)
        q = (st.S2 / n).astype(F)
        v = (q - (m * m).astype(F)).astype(F)
        v = np.where(v < 0, F(0), v).astype(F)
        e = (tol * (m + dark).astype(F)).astype(F)
        return v <= ((e * e).astype(F) * n).astype(F)


def select(st: State, p: Params) -> np.ndarray:
    """the sorted indices of the pixels with issued < max_samples that are not converged"""
    return np.nonzero((st.issued < p.max_samples) & ~converged(st, p.tolerance, p.dark))[0]


def call(st: State, p: Params, results, t_sky=None):
    """One bhray_accum_add_adaptive call.  results[s]: the (npix, 4) trace results of sample s for ALL pixels (only the pixels that take sample s are read).
    Returns (info, actives): info as bhray_accum_adaptive_info, actives the pixel set of every round after the first."""
    assert p.min_samples >= 2 and p.max_samples >= p.min_samples and p.round_samples >= 1 and (p.max_samples - p.min_samples) % p.round_samples == 0
    npix = st.issued.size
    info = {"rounds": 0, "active_last": 0, "rays": 0, "reach": 0}
    actives = []

    def give(pix, count):
        for j in range(count):                                   # in increasing s, each pixel from its own issued
            s = st.issued[pix] + j
            for sv in np.unique(s):
                k = pix[s == sv]
                add_sample(st, k, A.resolve(np.asarray(results[int(sv)], F).reshape(-1, 4)[k], t_sky))
        st.issued[pix] += np.uint32(count)
        info["rounds"] += 1
        info["rays"] += int(pix.size) * count

    if st.mode is None:
        give(np.arange(npix), p.min_samples)
        st.mode = (p.min_samples, p.round_samples)
    assert st.mode == (p.min_samples, p.round_samples), "min_samples and round_samples must repeat the first call's"
    while True:
        pix = select(st, p)
        info["active_last"] = int(pix.size)
        if pix.size == 0:
            break
        actives.append(pix)
        give(pix, p.round_samples)
    info["reach"] = int(st.issued.max())
    return info, actives


def mean(st: State) -> np.ndarray:
    return A.mean(st.sum)
