"""The footprint-filtered sky pass (bhray_set_sky_filter) restated in NumPy, binary32 operation by operation: the mip pyramid of the sky texture
and the per-pixel filter, built from oracle.np_ray's own bh_atan2, sample_bilinear, mix and PI.  What tests/test_sky_filter_ref_cpu.py,
tests/test_sky_filter_host.py and tests/test_gpu_sky_filter.py compare with; profiles/sky_filter_cost.py takes its shares from it."""
from __future__ import annotations

import numpy as np

from oracle import np_ray as N

F = np.float32


def sizes(w: int, h: int):
    """[(w, h)] of every level, level 0 included: w[l+1] = (w[l] + 1) >> 1, the same for h, until both are 1"""
    out = [(int(w), int(h))]
    while out[-1] != (1, 1):
        a, b = out[-1]
        out.append(((a + 1) >> 1, (b + 1) >> 1))
    return out


def _down(src):
    """one level down: ((a + b) + (c + d)) * 0.25 over 2x2 blocks clamped to the last column and row; src (h, w, 3) float32 -> (h', w', 4) float16, alpha 1"""
    h, w = src.shape[:2]
    h2, w2 = (h + 1) >> 1, (w + 1) >> 1
    j = np.arange(h2)[:, None]; i = np.arange(w2)[None, :]
    x0, x1 = 2 * i, np.minimum(2 * i + 1, w - 1)
    y0, y1 = 2 * j, np.minimum(2 * j + 1, h - 1)
    a, b, c, d = src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]
    rgb = (((a + b) + (c + d)) * F(0.25)).astype(F)
    out = np.ones((h2, w2, 4), dtype=np.float16)
    out[..., 0:3] = rgb.astype(np.float16)
    return out


def pyramid(t_sky):
    """pyr[l] = level l: pyr[0] the RGBA8 texture itself, pyr[l >= 1] (h_l, w_l, 4) float16.  Level 1 averages radiance - (b / 255)^4 as the sky pass forms it -,
    level l + 1 >= 2 the stored, rounded halves of level l."""
    t = np.ascontiguousarray(t_sky, dtype=np.uint8)
    pyr = [t]
    r = t[..., 0:3].astype(F) / F(255.0)
    src = (r * r) * (r * r)
    while src.shape[:2] != (1, 1):
        lvl = _down(src)
        pyr.append(lvl)
        src = lvl[..., 0:3].astype(F)
    return pyr


def _coord(t, n):
    """bhray_tex.h unit_coord / np_ray.sample_bilinear's coord"""
    with np.errstate(invalid="ignore"):
        x = t * F(n) - F(0.5)
        x = np.where(~(x >= F(-1.0)), F(-1.0), x)
        x = np.where(x > F(n), F(n), x)
    fl = np.floor(x)
    a = fl.astype(np.int64); b = a + 1
    return np.clip(a, 0, n - 1), np.clip(b, 0, n - 1), (x - fl).astype(F)


def sample_level(pyr, l: int, u, v):
    """S_l(u, v), (n, 3) float32: level 0 - the sky pass's bilinear sample of the RGBA8 texture, then ^4; level l >= 1 - the same coordinates and mix over that
    level's halves widened to binary32, clamp-to-edge, no power"""
    if l == 0:
        sc = N.sample_bilinear(pyr[0], u, v)[:, 0:3]
        return ((sc * sc) * (sc * sc)).astype(F)
    lv = pyr[l]
    h, w = lv.shape[:2]
    x0, x1, fx = _coord(np.asarray(u, dtype=F), w)
    y0, y1, fy = _coord(np.asarray(v, dtype=F), h)
    T = lv[..., 0:3].astype(F)
    a, b, c, d = T[y0, x0], T[y0, x1], T[y1, x0], T[y1, x1]
    top = N.mix(a, b, fx[..., None]); bot = N.mix(c, d, fx[..., None])
    return N.mix(top, bot, fy[..., None]).astype(F)


def uv(d):
    """sky_kernel's (u, v) of a direction (n, 3): the two bh_atan2, the divisions, the truncf"""
    with np.errstate(invalid="ignore", over="ignore"):
        theta = N.bh_atan2(np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]), d[:, 1])
        phi = N.bh_atan2(d[:, 2], d[:, 0])
        u = (phi + F(2.6) * N.PI) / (F(2.0) * N.PI)
        v = (N.PI - theta) / N.PI
        u = u - np.trunc(u); v = v - np.trunc(v)
    return u.astype(F), v.astype(F)


def level_and_fraction(rho):
    """(L, f) of a filter width rho >= 1: L the unbiased exponent, f = rho * 2^-L - 1 (exact, in [0, 1))"""
    rho = np.asarray(rho, dtype=F)
    L = ((rho.view(np.uint32) >> 23) & 255).astype(np.int64) - 127
    f = (rho * np.ldexp(F(1.0), -L).astype(F) - F(1.0)).astype(F)
    return L, f


def _neighbour(D, isdir, axis):
    """the one-sided difference along `axis` (1: x, 0: y): (delta (h, w, 3), uses_second (h, w) bool, none (h, w) bool)"""
    h, w = isdir.shape
    first = np.zeros((h, w), bool); second = np.zeros((h, w), bool)
    nf = np.zeros_like(D); ns = np.zeros_like(D)
    if axis == 1:
        first[:, :-1] = isdir[:, 1:]; nf[:, :-1] = D[:, 1:]
        second[:, 1:] = isdir[:, :-1]; ns[:, 1:] = D[:, :-1]
    else:
        first[:-1, :] = isdir[1:, :]; nf[:-1, :] = D[1:, :]
        second[1:, :] = isdir[:-1, :]; ns[1:, :] = D[:-1, :]
    second &= ~first
    n = np.where(first[..., None], nf, ns)
    with np.errstate(invalid="ignore", over="ignore"):
        delta = np.where((first | second)[..., None], n - D, F(0.0)).astype(F)
    return delta, second, ~(first | second)


def _len(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(F)


def resolve(frame_rgba32f, t_sky, pyr=None, enabled: bool = True):
    """(RGBA16F image, stats) of the sky pass with the footprint filter over an RGBA32F frame (h, w, 4).  enabled=False: no pixel is filtered - every direction pixel
    takes the one-tap path, which is sky_kernel's."""
    p = np.asarray(frame_rgba32f, dtype=F)
    h, w = p.shape[:2]
    sky_w = int(t_sky.shape[1])
    if pyr is None:
        pyr = pyramid(t_sky)
    with np.errstate(invalid="ignore"):
        isdir = p[..., 3] == 0
    D = p[..., 0:3]
    dh, left, none_h = _neighbour(D, isdir, 1)
    dv, up, none_v = _neighbour(D, isdir, 0)
    k = F(sky_w) / (F(2.0) * N.PI)
    with np.errstate(invalid="ignore", over="ignore"):
        rh = (_len(dh) * k).astype(F); rv = (_len(dv) * k).astype(F)
        hmaj = rh >= rv
        major = np.where(hmaj, rh, rv); minor = np.where(hmaj, rv, rh)
        delta = np.where(hmaj[..., None], dh, dv)
        filt = isdir & (major > F(1.0)) & (major < F(sky_w))
        if not enabled:
            filt = np.zeros_like(filt)
        mc = np.where(minor > F(1.0), minor, F(1.0)).astype(F)
        n_taps = np.full((h, w), 8, np.int64)
        for n in (4, 2, 1):
            n_taps = np.where(major <= (mc * F(n)) * F(1.5), n, n_taps)
        q = (major / n_taps.astype(F)).astype(F)
        rho = np.where(q > mc, q, mc).astype(F)
    n_taps = np.where(filt, n_taps, 1)
    rho = np.where(filt, rho, F(1.0)).astype(F)
    L, f = level_and_fraction(rho)

    idx = np.nonzero(isdir.ravel())[0]
    Df = D.reshape(-1, 3)[idx]; Del = delta.reshape(-1, 3)[idx]
    Nf = n_taps.ravel()[idx]; Lf = L.ravel()[idx]; ff = f.ravel()[idx]; flt = filt.ravel()[idx]
    acc = np.zeros((idx.size, 3), dtype=F)
    for t in range(8):
        m = np.nonzero(Nf > t)[0]
        if not m.size:
            break
        s = ((F(t) + F(0.5)) / Nf[m].astype(F) - F(0.5)).astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            dt = np.where(flt[m, None], Df[m] + (Del[m] * s[:, None]).astype(F), Df[m]).astype(F)
        u, v = uv(dt)
        T = np.zeros((m.size, 3), dtype=F)
        for l in np.unique(Lf[m]):
            g = np.nonzero(Lf[m] == l)[0]
            lo = sample_level(pyr, int(l), u[g], v[g])
            fr = ff[m][g]
            nz = fr != 0
            val = lo
            if nz.any():
                hi = sample_level(pyr, int(l) + 1, u[g][nz], v[g][nz])
                val = lo.copy()
                val[nz] = N.mix(lo[nz], hi, fr[nz][:, None]).astype(F)
            T[g] = val
        acc[m] = T if t == 0 else (acc[m] + T).astype(F)
    acc = (acc * (F(1.0) / Nf.astype(F))[:, None]).astype(F)

    out = p.reshape(-1, 4).copy()
    out[idx, 0:3] = acc
    out[idx, 3] = 1.0
    nf = int(filt.sum())
    stats = {
        "direction": int(isdir.sum()),
        "filtered": nf,
        "taps": {n: int((n_taps[filt] == n).sum()) for n in (1, 2, 4, 8)},
        "levels": {int(l): int((L[filt] == l).sum()) for l in np.unique(L[filt])},
        "frac_nonzero": int((f[filt] != 0).sum()),
        "left_fallback": int((isdir & left).sum()),
        "up_fallback": int((isdir & up).sum()),
        "isolated": int((isdir & none_h & none_v).sum()),
        "mask": filt,
    }
    with np.errstate(over="ignore"):
        return out.reshape(h, w, 4).astype(np.float16), stats


# the coverage tests/test_gpu_sky_filter.py asks of its 64 x 36 frame of the default scene with the 512 x 256 sky, so that the comparison hides no path:
# tests/test_sky_filter_ref_cpu.py shows that np_ray's frame of that scene meets it (the floors do not depend on the device)
FLOORS = dict(filtered=1800, taps={1: 1000, 2: 300, 4: 100, 8: 3}, levels=4, frac_nonzero=1500, left_fallback=40, up_fallback=80, isolated=2)


def check_floors(st, floors=FLOORS):
    assert st["filtered"] >= floors["filtered"], st
    for n, least in floors["taps"].items():
        assert st["taps"][n] >= least, (n, st["taps"])
    assert len(st["levels"]) >= floors["levels"], st["levels"]
    assert st["frac_nonzero"] >= floors["frac_nonzero"], st
    assert st["left_fallback"] >= floors["left_fallback"] and st["up_fallback"] >= floors["up_fallback"] and st["isolated"] >= floors["isolated"], st
