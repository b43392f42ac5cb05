"""The still cameras (bhray_accum_set_camera) restated in NumPy from include/bhray.h's contract, binary32 operation by operation: the rays of sample s
of every frame pixel under the pinhole, the equirectangular and the fisheye projection and under the thin lens.  Written from the contract, not from
bhusie_amd/cameras.py: it shares no function with cameras.still_rays (its own sine and cosine, hash, normalise and offsets), so that the two and the C text are
three statements of one rule.  What tests/test_still_camera_cpu.py and tests/test_gpu_still_camera.py compare with."""
from __future__ import annotations

import numpy as np

f = np.float32
PINHOLE, EQUIRECT, FISHEYE = 0, 1, 2
M32 = 0xFFFFFFFF


class Still:
    """the fields of a bhray_still_camera"""
    def __init__(self, projection=PINHOLE, fisheye_fov=3.14159274, lens_radius=0.0, focus_distance=1.0):
        self.projection, self.fisheye_fov, self.lens_radius, self.focus_distance = int(projection), f(fisheye_fov), f(lens_radius), f(focus_distance)


def _m(a, b):
    return np.multiply(a, b, dtype=f)


def _a(a, b):
    return np.add(a, b, dtype=f)


def _s(a, b):
    return np.subtract(a, b, dtype=f)


def _d(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.divide(a, b, dtype=f)


def sincos(x, cosine: bool):
    """the library's sine / cosine of binary32 arrays: Cody-Waite reduction by pi / 4 in three parts, two polynomials, every operation rounded"""
    xin = np.asarray(x, dtype=f)
    ax = np.abs(xin)
    neg = np.zeros(xin.shape, bool) if cosine else np.signbit(xin)
    assert (ax <= f(3.0e9)).all()
    j = _m(ax, f(1.27323954)).astype(np.int64)                    # truncation, as the conversion to uint32
    j = j + (j & 1)
    y = j.astype(f)
    r = _s(_s(_s(ax, _m(y, f(0.78515625))), _m(y, f(2.4187564849853515625e-4))), _m(y, f(3.77489497744594108e-8)))
    j = j & 7
    flip = j > 3
    neg = neg ^ flip
    j = np.where(flip, j - 4, j)
    if cosine:
        neg = neg ^ (j > 1)
    z = _m(r, r)
    mid = (j == 1) | (j == 2)
    use_cos = ~mid if cosine else mid
    pc = f(2.443315711809948e-5)
    pc = _s(_m(pc, z), f(1.388731625493765e-3))
    pc = _a(_m(pc, z), f(4.166664568298827e-2))
    vc = _a(_s(_m(_m(pc, z), z), _m(f(0.5), z)), f(1.0))
    ps = f(-1.9515295891e-4)
    ps = _a(_m(ps, z), f(8.3321608736e-3))
    ps = _s(_m(ps, z), f(1.6666654611e-1))
    vs = _a(_m(_m(ps, z), r), r)
    v = np.where(use_cos, vc, vs).astype(f)
    return np.where(neg, -v, v).astype(f)


def _dot3(a, b):
    return _a(_a(_m(a[..., 0], b[..., 0]), _m(a[..., 1], b[..., 1])), _m(a[..., 2], b[..., 2]))


def _unit(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = _d(f(1.0), np.sqrt(_dot3(v, v), dtype=f))
        return _m(v, np.asarray(inv)[..., None])


def _cross3(a, b):
    return np.array([_s(_m(a[1], b[2]), _m(a[2], b[1])), _s(_m(a[2], b[0]), _m(a[0], b[2])), _s(_m(a[0], b[1]), _m(a[1], b[0]))], dtype=f)


def offset(s: int):
    u = (0x80000000 + int(s) * 0xC13FA9A9) & M32
    v = (0x80000000 + int(s) * 0x91E10DA5) & M32
    return _s(_m(f(u >> 8), f(2.0 ** -24)), f(0.5)), _s(_m(f(v >> 8), f(2.0 ** -24)), f(0.5))


def frame_basis(camera_uniform: bytes):
    """(position, forward, fov, right, up, fwd_ff, fwd_n) from the 32 bytes of a camera uniform, as a frame forms them"""
    u = np.frombuffer(bytes(camera_uniform), dtype=f)
    pos, fwd, fov = u[0:3].copy(), u[4:7].copy(), f(u[7])
    right = _unit(_cross3(fwd, np.array([0.0, -1.0, 0.0], f)))
    up = _unit(_cross3(fwd, right))
    half = _d(fov, f(2.0))
    fov_factor = _d(f(1.0), _d(sincos(half, False), sincos(half, True)))
    return pos, fwd, fov, right, up, _m(fwd, fov_factor), _unit(fwd)


def hash32(v):
    v = np.asarray(v, dtype=np.uint64) & M32
    v ^= v >> 16
    v = (v * 0x7FEB352D) & M32
    v ^= v >> 15
    v = (v * 0x846CA68B) & M32
    v ^= v >> 16
    return v


def lens_uv(q, s: int):
    """(ru, rv) of level pixel index q and sample s (either may be an array; s < 2^16): the two rotated Kronecker sequences cut to 24 bits"""
    s = np.asarray(s, dtype=np.uint64)
    a = (hash32(q) + s * 0x9E3779B9) & M32
    b = (hash32(np.asarray(q, dtype=np.uint64) ^ 0x9E3779B9) + s * 0x6A09E667) & M32
    return _m((a >> 8).astype(f), f(2.0 ** -24)), _m((b >> 8).astype(f), f(2.0 ** -24))


def sample_rays(camera_uniform: bytes, cfg, still: Still | None, s: int) -> np.ndarray:
    """the (frame_h * frame_w, 8) records of sample s: row 0 the top, x fastest"""
    st = still if still is not None else Still()
    lw, lh = int(cfg.level_w[cfg.levels - 1]), int(cfg.level_h[cfg.levels - 1])
    w, h, cx, cy = int(cfg.frame_w), int(cfg.frame_h), int(cfg.crop_x), int(cfg.crop_y)
    pos, _, _, right, up, fwd_ff, fwd_n = frame_basis(camera_uniform)
    dx, dy = offset(s)
    lx, ly = np.meshgrid(np.arange(cx, cx + w), np.arange(cy, cy + h))         # (h, w): the level pixel of every frame pixel
    px, py = _a(lx.astype(f), dx), _a(ly.astype(f), dy)
    half_w, half_h = _m(f(lw - 1), f(0.5)), _m(f(lh - 1), f(0.5))
    origin = np.broadcast_to(pos, (h, w, 3)).astype(f)
    if st.projection == EQUIRECT:
        lon = _m(_s(px, half_w), _d(f(6.28318548), f(lw)))
        lat = _m(_s(py, half_h), _d(f(3.14159274), f(lh)))
        cl, sl, cp, sp = sincos(lon, True), sincos(lon, False), sincos(lat, True), sincos(lat, False)
        v = _a(_a(_m(fwd_n, _m(cp, cl)[..., None]), _m(right, _m(cp, sl)[..., None])), _m(up, sp[..., None]))
        direction = _unit(v)
    elif st.projection == FISHEYE:
        radius = _m(f(min(lw - 1, lh - 1)), f(0.5))
        X, Y = _d(_s(px, half_w), radius), _d(_s(py, half_h), radius)
        r = np.sqrt(_a(_m(X, X), _m(Y, Y)), dtype=f)
        theta = _m(r, _m(st.fisheye_fov, f(0.5)))
        safe = np.where(r > f(0.0), r, f(1.0)).astype(f)
        cphi, sphi = _d(X, safe), _d(Y, safe)
        sn, cs = sincos(theta, False), sincos(theta, True)
        v = _a(_a(_m(fwd_n, cs[..., None]), _m(right, _m(sn, cphi)[..., None])), _m(up, _m(sn, sphi)[..., None]))
        direction = np.where((r <= f(1.0))[..., None], _unit(v), f(0.0)).astype(f)
    else:
        assert st.projection == PINHOLE
        inc = _d(f(1.0), f(min(lw - 1, lh - 1)))
        posx = _m(_m(f(2.0), _s(px, half_w)), inc)
        posy = _m(_m(f(2.0), _s(py, half_h)), inc)
        direction = _unit(_a(_a(_m(right, posx[..., None]), _m(up, posy[..., None])), fwd_ff))
        if st.lens_radius > 0:
            q = (ly.astype(np.uint64) * lw + lx.astype(np.uint64)) & M32
            ru, rv = lens_uv(q, s)
            rr = np.sqrt(ru, dtype=f)
            ang = _m(rv, f(6.28318548))
            ex = _m(_m(rr, sincos(ang, True)), st.lens_radius)
            ey = _m(_m(rr, sincos(ang, False)), st.lens_radius)
            off = _a(_m(right, ex[..., None]), _m(up, ey[..., None]))
            origin = _a(origin, off)
            direction = _unit(_s(_m(direction, st.focus_distance), off))
    out = np.zeros((h * w, 8), dtype=f)
    out[:, 0:3] = origin.reshape(-1, 3)
    out[:, 4:7] = direction.reshape(-1, 3)
    return out
