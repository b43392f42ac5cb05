"""The accumulation image (bhray_accum_*) restated in NumPy, binary32 operation by operation: the sample offsets, the rays of a sample, the sky resolve
without its binary16 store, the sum in sample order and the mean.  What tests/test_accum_ref_cpu.py, tests/test_accum_host.py and tests/test_gpu_accum.py compare with."""
from __future__ import annotations

import numpy as np

from bhusie_amd import cameras
from oracle import np_ray as N

F = np.float32
MAX_SAMPLES = 65536


def offset(s: int):
    """(dx, dy) of sample s: u = 0x80000000 + s * 0xC13FA9A9, v = 0x80000000 + s * 0x91E10DA5 (mod 2^32); float(u >> 8) * 2^-24 - 0.5, every step exact"""
    u = (0x80000000 + int(s) * 0xC13FA9A9) % (1 << 32)
    v = (0x80000000 + int(s) * 0x91E10DA5) % (1 << 32)
    dx = F(F(F(u >> 8) * F(2.0 ** -24)) - F(0.5))
    dy = F(F(F(v >> 8) * F(2.0 ** -24)) - F(0.5))
    # exactness: the same numbers in rational arithmetic
    assert float(dx) == (u >> 8) / 2.0 ** 24 - 0.5 and float(dy) == (v >> 8) / 2.0 ** 24 - 0.5
    return dx, dy


def sample_rays(camera, cfg, s: int) -> np.ndarray:
    """the (frame_h * frame_w, 8) records of sample s: create_ray on the ladder's last level at the frame's window, through (x + dx, y + dy)"""
    lw, lh = int(cfg.level_w[cfg.levels - 1]), int(cfg.level_h[cfg.levels - 1])
    return cameras.pinhole_rays(camera, int(cfg.frame_w), int(cfg.frame_h), offset=offset(s), level=(lw, lh), crop=(int(cfg.crop_x), int(cfg.crop_y)))


def resolve(results, t_sky) -> np.ndarray:
    """oracle.np_ray.sky_resolve without its final cast: alpha == 0 -> (sky^4, 1) in binary32; every other result passes through.  results: (n, 4)"""
    flat = np.asarray(results, dtype=F).reshape(-1, 4)
    out = flat.copy()
    with np.errstate(invalid="ignore"):
        k = np.nonzero(flat[:, 3] == 0)[0]
    if k.size:
        d = flat[k, :3]
        with np.errstate(invalid="ignore"):
            theta = N.bh_atan2(np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]), d[:, 1])
            phi = N.bh_atan2(d[:, 2], d[:, 0])
            u = (phi + N.f32(2.6) * N.PI) / (N.f32(2.0) * N.PI)
            v = (N.PI - theta) / N.PI
            u = u - np.trunc(u); v = v - np.trunc(v)
            sc = N.sample_bilinear(t_sky, u, v)[:, 0:3]
        out[k, 0:3] = (sc * sc) * (sc * sc)
        out[k, 3] = 1.0
    assert out.dtype == F
    return out


def taken(resolved) -> np.ndarray:
    """(n,) bool: the sample counts - r, g and b are finite"""
    return np.isfinite(resolved[:, 0:3]).all(axis=1)


def accumulate(per_sample_results, t_sky) -> np.ndarray:
    """sum over the samples in order: (n, 4) float32, .w = the samples taken.  per_sample_results: an iterable of (n, 4) trace results"""
    total = None
    for r in per_sample_results:
        c = resolve(r, t_sky)
        if total is None:
            total = np.zeros_like(c)
        ok = taken(c)
        add = np.concatenate([c[:, 0:3], np.ones((c.shape[0], 1), F)], axis=1)
        total[ok] = (total[ok] + add[ok]).astype(F)          # one rounded add per channel per sample
    return total


def mean(total) -> np.ndarray:
    """(sum.xyz / n, 1), n = sum.w; n == 0: zeros"""
    n = total[:, 3]
    out = np.zeros_like(total)
    ok = n != 0
    out[ok, 0:3] = (total[ok, 0:3] / n[ok, None]).astype(F)
    out[ok, 3] = 1.0
    return out
