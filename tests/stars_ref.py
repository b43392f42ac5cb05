"""The point-star pass (bhray_set_stars) restated in NumPy from the section's text: binary32, one rounded operation at a time, + - * / sqrt and
compares only.  resolve() is rules 1 - 6 over an RGBA32F frame (what bhray_stars_resolve_host and the kernel's per-pixel function compute), apply() is rule 7 over
an RGBA16F sky image.  The pixel loop is plain Python over the pixels that have a footprint: the frames of the tests are a few thousand pixels."""
import functools

import numpy as np

F = np.float32
MAX_CELLS = 64
EPS = F(2.0 ** -12)


def grid_size(n):
    g = 1
    while g < 1024 and 12 * g * g < n:
        g *= 2
    return g


def _coord(a, G):
    """floorf((a * 0.5f + 0.5f) * G) clamped to [0, G - 1]"""
    t = np.floor((np.asarray(a, F) * F(0.5) + F(0.5)) * F(G))
    return np.clip(t, F(0), F(G - 1)).astype(np.int64)


def cells(dirs, G):
    """rule 4: the cell of every direction of an (n, 3) float32 array"""
    d = np.asarray(dirs, F).reshape(-1, 3)
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    fx = (ax >= ay) & (ax >= az)
    fy = ~fx & (ay >= az)
    fz = ~fx & ~fy
    m = np.where(fx, ax, np.where(fy, ay, az))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(fx, d[:, 1], d[:, 0]) / m
        b = np.where(fz, d[:, 1], d[:, 2]) / m
    comp = np.where(fx, d[:, 0], np.where(fy, d[:, 1], d[:, 2]))
    face = np.where(fx, 0, np.where(fy, 2, 4)) + (comp < 0)
    return ((face * G + _coord(b, G)) * G + _coord(a, G)).astype(np.int64)


def build_index(stars):
    """(G, order, prefix): the stars' order by (cell, original index) and the cells' prefix array"""
    s = np.asarray(stars, F).reshape(-1, 6)
    G = grid_size(len(s))
    c = cells(s[:, 0:3], G)
    order = np.argsort(c, kind="stable")
    prefix = np.zeros(6 * G * G + 1, np.int64)
    np.add.at(prefix, c + 1, 1)
    return G, order, np.cumsum(prefix)


def corners(frame):
    """rule 1: ((h + 1, w + 1, 3) float32 corners, (h + 1, w + 1) validity)"""
    f = np.asarray(frame, F)
    h, w = f.shape[:2]
    with np.errstate(invalid="ignore"):
        ok = (f[..., 3] == 0) & np.isfinite(f[..., 0:3]).all(axis=-1)
    d = np.zeros((h + 2, w + 2, 3), F)
    d[1:-1, 1:-1] = f[..., 0:3]
    okp = np.zeros((h + 2, w + 2), bool)
    okp[1:-1, 1:-1] = ok
    with np.errstate(invalid="ignore", over="ignore"):
        c = ((d[:-1, :-1] + d[:-1, 1:]) + (d[1:, :-1] + d[1:, 1:])) * F(0.25)
    return c, okp[:-1, :-1] & okp[:-1, 1:] & okp[1:, :-1] & okp[1:, 1:]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def _box(f, cs, G):
    """rule 4 for one face: (a0, a1, b0, b1) or None"""
    axis, sgn = f >> 1, F(-1.0 if f & 1 else 1.0)
    m = [c[axis] * sgn for c in cs]
    if not all(v > 0 for v in m):
        return None
    ia, ib = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    a = [c[ia] / v for c, v in zip(cs, m)]
    b = [c[ib] / v for c, v in zip(cs, m)]
    alo, ahi, blo, bhi = min(a) - EPS, max(a) + EPS, min(b) - EPS, max(b) + EPS
    if not (alo <= 1 and ahi >= -1 and blo <= 1 and bhi >= -1):
        return None
    return int(_coord(alo, G)), int(_coord(ahi, G)), int(_coord(blo, G)), int(_coord(bhi, G))


def resolve(frame, stars, gain=1.0, min_area=1e-7, max_footprint=0.25):
    """(add, st): add (h, w, 4) float32 - acc * gain and, in alpha, the stars accepted; st: per-pixel arrays state (0 summed, 1 skipped by size, 2 skipped by cells,
    3 no footprint), faces, cells, tested, accepted, reversed, area, and hits = [(y, x, star index, reversed)]"""
    f = np.asarray(frame, F)
    s = np.asarray(stars, F).reshape(-1, 6)
    h, w = f.shape[:2]
    G, order, prefix = build_index(s)
    sd, sf = s[order, 0:3], s[order, 3:6]
    c, valid = corners(f)
    fp = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, :-1] & valid[1:, 1:]
    gain, min_area = F(gain), F(min_area)
    fp2 = F(max_footprint) * F(max_footprint)
    add = np.zeros((h, w, 4), F)
    st = {k: np.zeros((h, w), np.int64) for k in ("faces", "cells", "tested", "accepted", "reversed")}
    st["state"] = np.full((h, w), 3, np.int64)
    st["area"] = np.zeros((h, w), F)
    st["hits"] = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for y, x in np.argwhere(fp):
            c00, c10, c01, c11 = c[y, x], c[y, x + 1], c[y + 1, x], c[y + 1, x + 1]
            d = f[y, x, 0:3]
            # 2.
            g0, g1 = c11 - c00, c10 - c01
            chords = [_dot(e, e) for e in (c10 - c00, c11 - c10, c01 - c11, c00 - c01, g0, g1)]
            if not all(ch <= fp2 for ch in chords):
                st["state"][y, x] = 1
                continue
            # 3.
            n_ = _cross(g0, g1)
            A = F(0.5) * np.sqrt(_dot(n_, n_))
            inv = F(1.0) / (min_area if A < min_area else A)
            st["area"][y, x] = A
            # 4.
            cs = (c00, c10, c01, c11)
            boxes = [(fc, _box(fc, cs, G)) for fc in range(6)]
            boxes = [(fc, b) for fc, b in boxes if b is not None]
            total = sum((b[1] - b[0] + 1) * (b[3] - b[2] + 1) for _, b in boxes)
            st["faces"][y, x], st["cells"][y, x] = len(boxes), total
            if total > MAX_CELLS:
                st["state"][y, x] = 2
                continue
            st["state"][y, x] = 0
            # 5. and 6.
            nT, nR, nB, nL = _cross(c00, c10), _cross(c10, c11), _cross(c11, c01), _cross(c01, c00)
            acc = np.zeros(3, F)
            got = 0
            for fc, (a0, a1, b0, b1) in boxes:
                for bi in range(b0, b1 + 1):
                    row = (fc * G + bi) * G
                    for ai in range(a0, a1 + 1):
                        for k in range(prefix[row + ai], prefix[row + ai + 1]):
                            v = sd[k]
                            eT, eL, eB, eR = _dot(v, nT), _dot(v, nL), _dot(v, nB), _dot(v, nR)
                            fwd = eT >= 0 and eL >= 0 and eB > 0 and eR > 0
                            rev = eT <= 0 and eL <= 0 and eB < 0 and eR < 0
                            st["tested"][y, x] += 1
                            if not (fwd or rev) or not (_dot(v, d) > 0):
                                continue
                            acc = acc + sf[k] * inv
                            got += 1
                            st["reversed"][y, x] += (not fwd)
                            st["hits"].append((int(y), int(x), int(order[k]), not fwd))
            st["accepted"][y, x] = got
            add[y, x, 0:3] = acc * gain
            add[y, x, 3] = got
    return add, st


def apply(sky16, add):
    """rule 7: half(min(float(sky_half) + acc * gain, 65504)) on the colour channels of the pixels that accepted a star; everything else keeps its words"""
    out = np.array(sky16, dtype=np.float16, copy=True)
    m = add[..., 3] > 0
    with np.errstate(over="ignore", invalid="ignore"):
        v = out[m][:, 0:3].astype(F) + add[m][:, 0:3]
        v = np.where(F(65504.0) < v, F(65504.0), v)                  # min_(a, b) = b < a ? b : a
        px = out[m]
        px[:, 0:3] = v.astype(np.float16)
    out[m] = px
    return out


def floors(st):
    """the figures the coverage floors are about"""
    per_star = {}
    for y, x, k, _ in st["hits"]:
        per_star.setdefault(k, set()).add((y, x))
    return {"lit": int((st["accepted"] > 0).sum()), "reversed": int((st["reversed"] > 0).sum()), "two_stars": int((st["accepted"] >= 2).sum()),
            "max_stars": int(st["accepted"].max(initial=0)), "stars_in_two_pixels": sum(1 for v in per_star.values() if len(v) >= 2),
            "by_size": int((st["state"] == 1).sum()), "by_cells": int((st["state"] == 2).sum()), "footprints": int((st["state"] != 3).sum()),
            "two_faces": int(((st["state"] == 0) & (st["faces"] == 2)).sum()), "three_faces": int(((st["state"] == 0) & (st["faces"] == 3)).sum())}


# ---- the frames and catalogues the CPU and GPU tests share -------------------------------------------------------------------------------------------------------
TIE_W, TIE_H = 9, 7


def tie_frame(mirror=False, w=TIE_W, h=TIE_H):
    """Directions (x, y, 64) * 2^-6, all direction pixels: every corner, every cross product and every edge function of a star on the quarter-pixel grid is exact
    in binary32, so ties are ties.  (The factor is a power of two and changes no sign; without it a pixel's chord is 1, above the largest max_footprint, and no
    pixel would have a footprint.)  mirror: column x holds the direction of column w - 1 - x - the orientation of the images inside the Einstein ring."""
    f = np.zeros((h, w, 4), F)
    xs = np.arange(w, dtype=F)
    f[..., 0] = (xs[::-1] if mirror else xs)[None, :] / F(64)
    f[..., 1] = np.arange(h, dtype=F)[:, None] / F(64)
    f[..., 2] = 1
    return f


def tie_stars(points, flux=None):
    """stars at frame-plane positions (sx, sy) of tie_frame (pixel centres at integers), each with a flux of its own"""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    s = np.zeros((len(p), 6), F)
    s[:, 0], s[:, 1], s[:, 2] = p[:, 0] / 64.0, p[:, 1] / 64.0, 1.0
    s[:, 3:6] = (np.arange(len(p))[:, None] * 3 + np.arange(3)[None, :] + 1) * 2.0 ** -20 if flux is None else flux
    return s


def tie_owner(sx, sy, mirror=False, w=TIE_W):
    """The pixel (x, y) rule 5 names for a star at (sx, sy): the top and left edges are the closed ones, in frame order."""
    y = int(np.floor(sy + 0.5))
    return (w - 1 - int(np.ceil(sx - 0.5)) if mirror else int(np.floor(sx + 0.5))), y


def tie_points():
    """corners, edge midpoints of both kinds and centres, all inside the region that has footprints"""
    pts = []
    for x, y in ((2, 2), (3, 4), (6, 2), (7, 5), (4, 3)):
        pts += [(x - 0.5, y - 0.5), (x, y - 0.5), (x - 0.5, y), (x, y)]
    return pts


def crowded_catalogue(d0, n=2000, seed=7):
    """n stars inside the index cell (G of n stars) that holds direction d0, on a fine lattice over the cell's interior"""
    G = grid_size(n)
    d0 = np.asarray(d0, F)
    axis = int(np.argmax(np.abs(d0)))
    sgn = 1.0 if d0[axis] > 0 else -1.0
    ia, ib = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    m = abs(float(d0[axis]))
    ca, cb = int(_coord(d0[ia] / F(m), G)), int(_coord(d0[ib] / F(m), G))
    rng = np.random.default_rng(seed)
    t = rng.random((n, 2)) * 0.9 + 0.05
    a = ((ca + t[:, 0]) / G) * 2.0 - 1.0
    b = ((cb + t[:, 1]) / G) * 2.0 - 1.0
    s = np.zeros((n, 6), F)
    s[:, axis], s[:, ia], s[:, ib] = sgn, a, b
    s[:, 3:6] = (rng.random((n, 3)) * 1e-6 + 1e-7)
    assert len(set(cells(s[:, 0:3], G).tolist())) == 1
    return s


SEED = 1
DIAG_CAMERA = dict(position=(-11.0, -11.0, -11.0), forward=(1.0, 1.0, 1.0))


def scene(name):
    """(camera, black hole) of the named scene: default, nodisk (accretion_disk_outer = accretion_disk_inner), diag (disk-less, looking along (1, 1, 1))"""
    import bhusie_amd as B
    bh = B.BlackHole() if name == "default" else B.BlackHole(accretion_disk_outer=2.0, accretion_disk_inner=2.0)
    return (B.Camera(**DIAG_CAMERA) if name == "diag" else B.Camera()), bh


@functools.lru_cache(maxsize=None)
def catalogue():
    from bhusie_amd import assets
    return assets.star_catalogue(2000, SEED)


def check_floors(fl, name):
    """the coverage floors of DESIGN.md §23; `fl` is floors() of a 40 x 36 frame of scene `name` (crowded: the default scene under crowded_catalogue)"""
    if name == "default":
        assert fl["lit"] >= 40 and fl["reversed"] >= 10 and fl["two_stars"] >= 1 and fl["stars_in_two_pixels"] >= 5, fl
    elif name == "nodisk":
        assert fl["by_size"] >= 5, fl
    elif name == "diag":
        assert fl["two_faces"] >= 20 and fl["three_faces"] >= 3, fl
    elif name == "crowded":
        assert fl["max_stars"] >= 8, fl
