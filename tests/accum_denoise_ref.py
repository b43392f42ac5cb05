"""The denoised stills (bhray_accum_read_denoised) restated in NumPy from include/bhray.h's rule, binary32 operation by operation: validity, the
compressed luminance, the stop function, and the a-trous iterations with their 25 taps in the rule's order.  What tests/test_accum_denoise_host.py and
tests/test_gpu_accum_denoise.py compare with."""
from __future__ import annotations

import numpy as np

F = np.float32
COVERAGE, GEOMETRY, POSITION, ESCAPE, ALL = 1, 2, 4, 8, 0xF
PASSES = (COVERAGE, GEOMETRY, POSITION, ESCAPE)
H = (F(0.375), F(0.25), F(0.0625))


def valid(c) -> np.ndarray:
    """(h, w) bool: alpha == 1 and x, y, z finite"""
    with np.errstate(invalid="ignore"):
        return (c[..., 3] == F(1.0)) & np.isfinite(c[..., 0:3]).all(axis=-1)


def luminance(c) -> np.ndarray:
    """t: Y = (0.2126 r + 0.7152 g) + 0.0722 b; Y < 0 ? 0; Y >= 2^100 ? 1 : Y / (1 + Y) - one rounded operation each"""
    with np.errstate(all="ignore"):
        r, g, b = c[..., 0].astype(F), c[..., 1].astype(F), c[..., 2].astype(F)
        y = ((F(0.2126) * r).astype(F) + (F(0.7152) * g).astype(F)).astype(F)
        y = (y + (F(0.0722) * b).astype(F)).astype(F)
        y = np.where(y < 0, F(0.0), y).astype(F)
        return np.where(y >= F(2.0 ** 100), F(1.0), (y / (F(1.0) + y).astype(F)).astype(F)).astype(F)


def stop(d2, s2) -> np.ndarray:
    """E(d2, s2): q = d2 / s2; u = 1 - q; u > 0 ? u * u : 0 (a NaN gives 0)"""
    with np.errstate(all="ignore"):
        q = (d2.astype(F) / F(s2)).astype(F)
        u = (F(1.0) - q).astype(F)
        return np.where(u > 0, (u * u).astype(F), F(0.0)).astype(F)


def dist2(p, q) -> np.ndarray:
    with np.errstate(all="ignore"):
        dx, dy, dz = (p[..., 0] - q[..., 0]).astype(F), (p[..., 1] - q[..., 1]).astype(F), (p[..., 2] - q[..., 2]).astype(F)
        return (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)


def _shift(img, a, b, fill):
    """out[y, x] = img[y + b, x + a], `fill` where that lies outside the frame"""
    h, w = img.shape[0], img.shape[1]
    out = np.full_like(img, fill)
    ys0, ys1 = max(0, -b), min(h, h - b)
    xs0, xs1 = max(0, -a), min(w, w - a)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = img[ys0 + b:ys1 + b, xs0 + a:xs1 + a]
    return out


def sigma2(params) -> dict:
    """each s2 = sigma * sigma in binary32"""
    return {k: F(F(params[k]) * F(params[k])) for k in ("sigma_colour", "sigma_coverage", "sigma_closest", "sigma_position", "sigma_escape")}


def denoise(colour, guides: dict, params: dict) -> np.ndarray:
    """colour: (h, w, 4) float32, C_0; guides: {pass bit: (h, w, 4) float32 mean}, the set; params: iterations, guides (0: the whole set) and the five sigmas.
    Returns C_iterations."""
    with np.errstate(all="ignore"):
        s2 = sigma2(params)
    use = int(params.get("guides", 0)) or sum(guides)
    assert use and all((use >> i) & 1 == 0 or (1 << i) in guides for i in range(4))
    cur = np.array(colour, dtype=F, copy=True)
    h, w = cur.shape[:2]
    for it in range(int(params["iterations"])):
        step = 1 << it
        ok = valid(cur)
        t = luminance(cur)
        acc = np.zeros((h, w, 3), F)
        ws = np.zeros((h, w), F)
        with np.errstate(all="ignore"):
            for b in range(-2, 3):
                for a in range(-2, 3):
                    q_ok = _shift(ok, a * step, b * step, False)
                    wgt = np.full((h, w), F(H[abs(a)] * H[abs(b)]), F)
                    dt = (t - _shift(t, a * step, b * step, F(0))).astype(F)
                    wgt = (wgt * stop((dt * dt).astype(F), s2["sigma_colour"])).astype(F)
                    if use & COVERAGE:
                        m = guides[COVERAGE]
                        wgt = (wgt * stop(dist2(m, _shift(m, a * step, b * step, F(0))), s2["sigma_coverage"])).astype(F)
                    if use & GEOMETRY:
                        m = guides[GEOMETRY][..., 0]
                        d = (m - _shift(m, a * step, b * step, F(0))).astype(F)
                        wgt = (wgt * stop((d * d).astype(F), s2["sigma_closest"])).astype(F)
                    if use & POSITION:
                        m = guides[POSITION]
                        wgt = (wgt * stop(dist2(m, _shift(m, a * step, b * step, F(0))), s2["sigma_position"])).astype(F)
                    if use & ESCAPE:
                        m = guides[ESCAPE]
                        wgt = (wgt * stop(dist2(m, _shift(m, a * step, b * step, F(0))), s2["sigma_escape"])).astype(F)
                    take = ok & q_ok                              # a skipped tap adds nothing - not even w * 0
                    cq = _shift(cur[..., 0:3], a * step, b * step, F(0))
                    for ch in range(3):
                        acc[..., ch] = np.where(take, (acc[..., ch] + (wgt * cq[..., ch]).astype(F)).astype(F), acc[..., ch])
                    ws = np.where(take, (ws + wgt).astype(F), ws)
            new = cur.copy()
            hit = ok & (ws > 0)
            for ch in range(3):
                new[..., ch] = np.where(hit, (acc[..., ch] / ws).astype(F), cur[..., ch])
        # (np.where keeps the bits of what it passes through: a pixel that is not valid, or whose taps all weigh 0, keeps its value bit for bit)
        cur = new
    return cur
