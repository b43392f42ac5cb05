"""The still passes (bhray_accum_set_passes) restated in NumPy from include/bhray.h's contract, binary32 operation by operation: a sample's (v, 1) in
each pass, the sum in sample order - the box's, or the stencil of tests/accum_filter_ref.py - and the mean.  What tests/test_accum_passes_ref_cpu.py,
tests/test_accum_passes_host.py and tests/test_gpu_accum_passes.py compare with."""
from __future__ import annotations

import numpy as np

from tests import accum_filter_ref as FR
from tests import accum_ref as A

F = np.float32
COVERAGE, GEOMETRY, POSITION, ESCAPE, ALL = 1, 2, 4, 8, 0xF
PASSES = (COVERAGE, GEOMETRY, POSITION, ESCAPE)
NAMES = {"coverage": COVERAGE, "geometry": GEOMETRY, "position": POSITION, "escape": ESCAPE}
NONE, HORIZON, DISK, MESH, UNUSABLE = 0, 1, 2, 3, 255


def taken(results) -> np.ndarray:
    """(n,) bool: R.x, R.y and R.z are finite - the passes' own rule, on the trace's result alone"""
    r = np.asarray(results, dtype=F).reshape(-1, 4)
    return np.isfinite(r[:, 0:3]).all(axis=1)


def kinds(records) -> np.ndarray:
    return (np.asarray(records)["hit"] & 0xFF).astype(np.int64)


def values(results, records, rays, pass_bit: int) -> np.ndarray:
    """(n, 4) float32: (v, 1) of every taken sample, zeros for a skipped one.  results (n, 4); records: n of RAY_RECORD_DTYPE; rays (n, 8), read for ESCAPE only
    (None otherwise)."""
    assert pass_bit in PASSES
    r = np.asarray(results, dtype=F).reshape(-1, 4)
    q = np.asarray(records).reshape(-1)
    n = r.shape[0]
    kind = kinds(q)
    v = np.zeros((n, 4), F)
    if pass_bit == COVERAGE:
        for ch, k in enumerate((HORIZON, DISK, MESH)):
            v[:, ch] = (kind == k).astype(F)
    elif pass_bit == GEOMETRY:
        v[:, 0] = q["closest"]
        v[:, 1] = q["iterations"].astype(F)                      # uint32 -> binary32: one round-to-nearest-even
        v[:, 2] = q["transmittance"]
    elif pass_bit == POSITION:
        solid = (kind == DISK) | (kind == MESH)
        v[solid, 0:3] = q["position"][solid]
    else:
        d = np.asarray(rays, dtype=F).reshape(-1, 8)[:, 4:7]
        with np.errstate(invalid="ignore"):
            left = r[:, 3] == 0                                   # -0.0 too
        v[left, 0:3] = r[left, 0:3]
        straight = ~left & (kind == NONE)
        v[straight, 0:3] = d[straight]
    v[kind == UNUSABLE, 0:3] = 0.0                                # a finite black sample with a zero vector in every pass
    v[:, 3] = 1.0
    v[~taken(r)] = 0.0
    return v


def accumulate(per_sample, pass_bit: int, filt: FR.Filter | None = None, w: int = 0, h: int = 0, s0: int = 0) -> np.ndarray:
    """The sum over the samples in order: (n, 4) float32, .w the samples (the weight) taken.  per_sample: an iterable of (results, records, rays).  filt None or the
    box: total = total + (v, 1) where the sample is taken; a tent or a cubic: the stencil of tests/accum_filter_ref.py over V = values() as an (h, w) image."""
    boxed = filt is None or filt.kind == FR.BOX
    total = None
    for j, (results, records, rays) in enumerate(per_sample):
        v = values(results, records, rays, pass_bit)
        if total is None:
            total = np.zeros_like(v)
        if boxed:
            ok = v[:, 3] != 0
            total[ok] = (total[ok] + v[ok]).astype(F)            # one rounded add per channel per sample
        else:
            wx, wy = FR.weights(filt, s0 + j)
            with np.errstate(over="ignore", invalid="ignore"):
                total = (total + FR.stencil(v.reshape(h, w, 4), wx, wy).reshape(-1, 4)).astype(F)
    return total


def mean(total) -> np.ndarray:
    """(sum.xyz / w, 1); w == 0: zeros - the colour's operation"""
    return A.mean(total)
