"""Ray generators for RayPass.trace_rays / Renderer.render_rays (bhray_trace_rays): pure NumPy, binary32 arithmetic.

Each returns an (h * w, 8) float32 array of ray records - origin, pad, direction, pad (layouts.BhrayRay) - row 0 the top row, x fastest, as a frame's pixels.

pinhole_rays    the shader's create_ray (ray.wgsl:269-285), operation by operation: the rays of a `levels = 1` frame, bit for bit
equirect_rays   a 360 x 180 degree panorama: the centre column looks along `forward`
fisheye_rays    an equidistant fisheye of opening angle `fov` about `forward`; pixels outside the image circle get a zero direction (not traced: alpha -1)
still_rays      the rays of sample s of the accumulation image under a StillCamera (bhray_accum_set_camera): what the device generates, bit for bit
boost_rays      any of these records seen by a moving Observer: Lorentz aberration of the directions and the beam factors D^4, bit for bit

All three use create_ray's basis: plane_up = (0, -1, 0), right = normalize(cross(forward, plane_up)), up = normalize(cross(forward, right)) - `up` is the direction in
which the image's rows increase.  Directions are unit as a binary32 normalise leaves them (v * (1 / sqrt(dot(v, v)))), which is what the trace kernels expect.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
_PI = F(3.14159274)


def _dot(a, b):                                       # N1: (x*x + y*y) + z*z, one rounding per operation
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F)


def _normalize(a):                                    # N2: v * (1 / length(v))
    r = F(1.0) / np.sqrt(_dot(a, a), dtype=F)
    return (a * np.asarray(r, dtype=F)[..., None]).astype(F)


def _sincos(xin, kind):
    """bh_sincos<kind> of bhray_math.h for one binary32 value (kind 0: sin, 1: cos), operation by operation"""
    xin = F(xin)
    x = F(abs(xin))
    sign = bool(np.signbit(xin)) if kind == 0 else False
    if not x <= F(3.0e9):
        return F(np.nan)
    j = int(x * F(1.27323954)) & 0xFFFFFFFF
    j = j + (j & 1)
    y = F(j)
    x = F(F(F(x - F(y * F(0.78515625))) - F(y * F(2.4187564849853515625e-4))) - F(y * F(3.77489497744594108e-8)))
    j &= 7
    if j > 3:
        sign = not sign
        j -= 4
    if kind == 1 and j > 1:
        sign = not sign
    z = F(x * x)
    mid = j in (1, 2)
    use_cos = mid if kind == 0 else not mid
    if use_cos:
        p = F(2.443315711809948e-5)
        p = F(F(p * z) - F(1.388731625493765e-3))
        p = F(F(p * z) + F(4.166664568298827e-2))
        r = F(F(F(F(p * z) * z) - F(F(0.5) * z)) + F(1.0))
    else:
        p = F(-1.9515295891e-4)
        p = F(F(p * z) + F(8.3321608736e-3))
        p = F(F(p * z) - F(1.6666654611e-1))
        r = F(F(F(p * z) * x) + x)
    return F(-r) if sign else r


def _tan(x):                                          # bh_tan: ray.wgsl:279 under N4
    return F(_sincos(x, 0) / _sincos(x, 1))


def _basis(forward):
    fwd = np.asarray(forward, dtype=F).reshape(3)
    right = _normalize(_cross(fwd, np.array([0.0, -1.0, 0.0], dtype=F)))
    up = _normalize(_cross(fwd, right))
    return fwd, right, up


def _records(position, dirs):
    n = dirs.shape[0]
    out = np.zeros((n, 8), dtype=F)
    out[:, 0:3] = np.asarray(position, dtype=F).reshape(3)
    out[:, 4:7] = dirs
    return out


def _camera_fields(camera):
    """(position, forward, fov) as binary32 from a scene.Camera (through its uniform: the bytes the ctx gets) or from the 32 uniform bytes themselves"""
    b = camera if isinstance(camera, (bytes, bytearray)) else camera.uniform()
    u = np.frombuffer(bytes(b), dtype=F)
    assert u.size == 8, "a CameraUniform is 32 bytes"
    return u[0:3].copy(), u[4:7].copy(), F(u[7])


def r2_offset(s: int):
    """(dx, dy) of sample s of the accumulation image (bhray_accum_sample_offset): the R2 sequence in 32-bit integer arithmetic, cut to 24 bits so
    that every step is exact in binary32.  Sample 0: (0, 0), the pixel centre; every offset lies in [-0.5, 0.5)."""
    s = int(s)
    u = (0x80000000 + s * 0xC13FA9A9) & 0xFFFFFFFF
    v = (0x80000000 + s * 0x91E10DA5) & 0xFFFFFFFF
    return F(F(F(u >> 8) * F(2.0 ** -24)) - F(0.5)), F(F(F(v >> 8) * F(2.0 ** -24)) - F(0.5))


def pinhole_rays(camera, w: int, h: int, pixel=None, offset=(0.0, 0.0), level=None, crop=(0, 0)) -> np.ndarray:
    """create_ray for every pixel of a w x h level (ray.wgsl:269-285).  pixel=(x, y): that one pixel's ray only, as a (1, 8) array - the same
    arithmetic, so the same bits as row y * w + x of the whole level (Renderer.pick).
    offset=(dx, dy): the rays through (x + dx, y + dy) instead of the pixel centres, one rounded add per coordinate (r2_offset: the accumulation image's samples;
    (0, 0) changes no bit).  level=(lw, lh), crop=(cx, cy): the w x h pixels are the window at (cx, cy) of an lw x lh level, whose geometry the rays take
    (a cropped frame on its ladder's last level)."""
    w, h = int(w), int(h)
    lw, lh = (w, h) if level is None else (int(level[0]), int(level[1]))
    cx, cy = int(crop[0]), int(crop[1])
    assert lw >= 2 and lh >= 2, "create_ray divides by min(w, h) - 1"
    assert cx >= 0 and cy >= 0 and cx + w <= lw and cy + h <= lh, "pinhole_rays: the window leaves the level"
    pos, forward, fov = _camera_fields(camera)
    fwd, right, up = _basis(forward)
    sm = min(lw - 1, lh - 1)
    increment = F(1.0) / F(sm)
    px = (np.arange(cx, cx + w, dtype=F) + F(offset[0])).astype(F)[None, :]
    py = (np.arange(cy, cy + h, dtype=F) + F(offset[1])).astype(F)[:, None]
    if pixel is not None:
        x, y = int(pixel[0]), int(pixel[1])
        assert 0 <= x < w and 0 <= y < h, "pinhole_rays: the pixel lies outside the level"
        px, py = px[:, x:x + 1], py[y:y + 1, :]
        w, h = 1, 1
    posx = (F(2.0) * (px - F(F(lw - 1) * F(0.5)))) * increment
    posy = (F(2.0) * (py - F(F(lh - 1) * F(0.5)))) * increment
    posx = np.broadcast_to(posx, (h, w)).astype(F)
    posy = np.broadcast_to(posy, (h, w)).astype(F)
    fov_factor = F(F(1.0) / _tan(F(fov / F(2.0))))
    fwd_ff = (fwd * fov_factor).astype(F)
    v = ((right[None, None, :] * posx[..., None]).astype(F) + (up[None, None, :] * posy[..., None]).astype(F)).astype(F) + fwd_ff[None, None, :]
    return _records(pos, _normalize(v.astype(F)).reshape(h * w, 3))


def equirect_rays(position, forward, w: int, h: int) -> np.ndarray:
    """360 x 180 degrees, pixel centres: column i at longitude (i - (w - 1) / 2) * 2 pi / w from `forward` towards `right`, row j at latitude
    (j - (h - 1) / 2) * pi / h towards `up` (the image's downward direction, as in create_ray: row 0 is the top)."""
    w, h = int(w), int(h)
    assert w >= 1 and h >= 1
    fwd, right, up = _basis(forward)
    fwd = _normalize(fwd)
    lon = (np.arange(w, dtype=F) - F(F(w - 1) * F(0.5))) * F(F(2.0) * _PI / F(w))
    lat = (np.arange(h, dtype=F) - F(F(h - 1) * F(0.5))) * F(_PI / F(h))
    cl, sl = np.cos(lon, dtype=F)[None, :], np.sin(lon, dtype=F)[None, :]
    cp, sp = np.cos(lat, dtype=F)[:, None], np.sin(lat, dtype=F)[:, None]
    a = (cp * cl).astype(F)[..., None]
    b = (cp * sl).astype(F)[..., None]
    c = np.broadcast_to(sp, (h, w)).astype(F)[..., None]
    v = ((fwd * a).astype(F) + (right * b).astype(F)).astype(F) + (up * c).astype(F)
    return _records(position, _normalize(v.astype(F)).reshape(h * w, 3))


def fisheye_rays(position, forward, w: int, h: int, fov: float) -> np.ndarray:
    """Equidistant fisheye: a pixel at distance r from the image centre - in units of the image circle's radius min(w - 1, h - 1) / 2 - looks fov / 2 * r away from
    `forward`, in the image direction it lies in.  r > 1: outside the circle, direction zero."""
    w, h = int(w), int(h)
    assert w >= 2 and h >= 2
    fwd, right, up = _basis(forward)
    fwd = _normalize(fwd)
    radius = F(F(min(w - 1, h - 1)) * F(0.5))
    x = np.broadcast_to(((np.arange(w, dtype=F) - F(F(w - 1) * F(0.5))) / radius)[None, :], (h, w)).astype(F)
    y = np.broadcast_to(((np.arange(h, dtype=F) - F(F(h - 1) * F(0.5))) / radius)[:, None], (h, w)).astype(F)
    r = np.sqrt((x * x + y * y).astype(F), dtype=F)
    inside = r <= F(1.0)
    theta = (r * F(F(fov) * F(0.5))).astype(F)
    safe = np.where(r > F(0.0), r, F(1.0)).astype(F)
    cphi, sphi = (x / safe).astype(F), (y / safe).astype(F)           # r == 0: the centre, sin(theta) = 0 - the image direction does not matter
    st, ct = np.sin(theta, dtype=F), np.cos(theta, dtype=F)
    v = ((fwd * ct[..., None]).astype(F) + (right * (st * cphi).astype(F)[..., None]).astype(F)).astype(F) + (up * (st * sphi).astype(F)[..., None]).astype(F)
    d = _normalize(v.astype(F))
    d = np.where(inside[..., None], d, F(0.0)).astype(F)
    return _records(position, d.reshape(h * w, 3))


STILL_PINHOLE, STILL_EQUIRECT, STILL_FISHEYE = 0, 1, 2         # BHRAY_STILL_*


@dataclass(frozen=True)
class StillCamera:
    """The camera model of the accumulation image (bhray_still_camera): StillCamera.pinhole(), .pinhole(lens_radius, focus_distance) - a thin lens
    with a spherical surface of focus -, .equirect() and .fisheye(fov).  Position, forward and the pinhole's fov stay the scene camera's."""
    projection: int = STILL_PINHOLE
    fisheye_fov: float = float(_PI)
    lens_radius: float = 0.0
    focus_distance: float = 1.0

    @classmethod
    def pinhole(cls, lens_radius: float = 0.0, focus_distance: float = 1.0) -> "StillCamera":
        return cls(STILL_PINHOLE, float(_PI), float(lens_radius), float(focus_distance))

    @classmethod
    def equirect(cls) -> "StillCamera":
        return cls(STILL_EQUIRECT)

    @classmethod
    def fisheye(cls, fov: float) -> "StillCamera":
        return cls(STILL_FISHEYE, float(fov))

    @property
    def is_default(self) -> bool:
        return self.projection == STILL_PINHOLE and not self.lens_radius > 0.0

    def struct(self):
        """the bhray_still_camera the library takes"""
        import ctypes as C
        from .layouts import BhrayStillCamera
        return BhrayStillCamera(C.sizeof(BhrayStillCamera), int(self.projection), float(self.fisheye_fov), float(self.lens_radius), float(self.focus_distance))


def _vsincos(x, kind):
    return np.array([_sincos(v, kind) for v in np.asarray(x, dtype=F).ravel()], dtype=F).reshape(np.shape(x))


def _still_hash(v):
    v = np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF
    v = v ^ (v >> 16)
    v = (v * 0x7FEB352D) & 0xFFFFFFFF
    v = v ^ (v >> 15)
    v = (v * 0x846CA68B) & 0xFFFFFFFF
    return v ^ (v >> 16)


def still_rays(camera, cfg, still_camera: StillCamera | None, s: int) -> np.ndarray:
    """The (frame_h * frame_w, 8) records of sample s of the accumulation image of `cfg` (a BhrayConfig) under `still_camera` (None: the default), every step of
    include/bhray.h's contract one rounded binary32 operation: r2_offset's sub-pixel offset, the projection on the ladder's last level at the frame's window, the
    lens point of the thin lens.  The pinhole without a lens is pinhole_rays(offset=..., level=..., crop=...)."""
    sc = still_camera if still_camera is not None else StillCamera()
    s = int(s)
    lw, lh = int(cfg.level_w[cfg.levels - 1]), int(cfg.level_h[cfg.levels - 1])
    w, h, cx, cy = int(cfg.frame_w), int(cfg.frame_h), int(cfg.crop_x), int(cfg.crop_y)
    dx, dy = r2_offset(s)
    if sc.projection == STILL_PINHOLE:
        rec = pinhole_rays(camera, w, h, offset=(dx, dy), level=(lw, lh), crop=(cx, cy))
        if not sc.lens_radius > 0.0:
            return rec
        pos, forward, _ = _camera_fields(camera)
        _, right, up = _basis(forward)
        q = ((np.arange(cy, cy + h, dtype=np.uint64)[:, None] * lw + np.arange(cx, cx + w, dtype=np.uint64)[None, :]) & 0xFFFFFFFF).reshape(-1)
        a = (_still_hash(q) + s * 0x9E3779B9) & 0xFFFFFFFF
        b = (_still_hash(q ^ 0x9E3779B9) + s * 0x6A09E667) & 0xFFFFFFFF
        ru = ((a >> 8).astype(F) * F(2.0 ** -24)).astype(F)
        rv = ((b >> 8).astype(F) * F(2.0 ** -24)).astype(F)
        rr = np.sqrt(ru, dtype=F)
        ang = (rv * F(6.28318548)).astype(F)
        ex = ((rr * _vsincos(ang, 1)).astype(F) * F(sc.lens_radius)).astype(F)
        ey = ((rr * _vsincos(ang, 0)).astype(F) * F(sc.lens_radius)).astype(F)
        off = ((right[None, :] * ex[:, None]).astype(F) + (up[None, :] * ey[:, None]).astype(F)).astype(F)
        out = rec.copy()
        out[:, 0:3] = (pos[None, :] + off).astype(F)
        out[:, 4:7] = _normalize(((rec[:, 4:7] * F(sc.focus_distance)).astype(F) - off).astype(F))
        return out
    pos, forward, _ = _camera_fields(camera)
    fwd, right, up = _basis(forward)
    fwd = _normalize(fwd)
    px = (np.arange(cx, cx + w, dtype=F) + dx).astype(F)
    py = (np.arange(cy, cy + h, dtype=F) + dy).astype(F)
    half_w, half_h = F(F(lw - 1) * F(0.5)), F(F(lh - 1) * F(0.5))
    if sc.projection == STILL_EQUIRECT:
        lon = ((px - half_w) * F(F(6.28318548) / F(lw))).astype(F)
        lat = ((py - half_h) * F(F(3.14159274) / F(lh))).astype(F)
        cl, sl = _vsincos(lon, 1)[None, :], _vsincos(lon, 0)[None, :]
        cp, sp = _vsincos(lat, 1)[:, None], _vsincos(lat, 0)[:, None]
        a = (cp * cl).astype(F)[..., None]
        b = (cp * sl).astype(F)[..., None]
        c = np.broadcast_to(sp, (h, w)).astype(F)[..., None]
        v = ((fwd * a).astype(F) + (right * b).astype(F)).astype(F) + (up * c).astype(F)
        return _records(pos, _normalize(v.astype(F)).reshape(h * w, 3))
    assert sc.projection == STILL_FISHEYE, "still_rays: unknown projection"
    radius = F(F(min(lw - 1, lh - 1)) * F(0.5))
    x = np.broadcast_to(((px - half_w) / radius).astype(F)[None, :], (h, w)).astype(F)
    y = np.broadcast_to(((py - half_h) / radius).astype(F)[:, None], (h, w)).astype(F)
    r = np.sqrt(((x * x).astype(F) + (y * y).astype(F)).astype(F), dtype=F)
    inside = r <= F(1.0)
    theta = (r * F(F(sc.fisheye_fov) * F(0.5))).astype(F)
    safe = np.where(r > F(0.0), r, F(1.0)).astype(F)
    cphi, sphi = (x / safe).astype(F), (y / safe).astype(F)
    st, ct = _vsincos(theta, 0), _vsincos(theta, 1)
    v = ((fwd * ct[..., None]).astype(F) + (right * (st * cphi).astype(F)[..., None]).astype(F)).astype(F) + (up * (st * sphi).astype(F)[..., None]).astype(F)
    d = _normalize(v.astype(F))
    d = np.where(inside[..., None], d, F(0.0)).astype(F)
    return _records(pos, d.reshape(h * w, 3))


@dataclass(frozen=True)
class Observer:
    """The moving observer of a still (bhray_observer): `velocity` is beta, the observer's velocity in the static frame, world axes, units of c
    (|beta| <= 0.99); beaming: also scale every sample by the bolometric D^4.  A zero velocity is no observer."""
    velocity: tuple = (0.0, 0.0, 0.0)
    beaming: bool = True

    @property
    def at_rest(self) -> bool:
        return all(F(v) == F(0.0) for v in self.velocity)

    def struct(self):
        """the bhray_observer the library takes"""
        import ctypes as C
        from .layouts import BhrayObserver
        vx, vy, vz = (float(v) for v in self.velocity)
        return BhrayObserver(C.sizeof(BhrayObserver), (C.c_float * 3)(vx, vy, vz), 1 if self.beaming else 0)


def boost_rays(rays, observer: Observer | None):
    """(rays', beam): the (n, 8) records `rays`, their directions given in the observer's rest frame, with the directions aberrated into the static frame, and the
    (n,) beam factors D^4 - include/bhray.h's rule (bhray_observer_boost_rays), one rounded binary32 operation at a time.  Origins are unchanged; an all-zero
    direction, a None observer or a zero velocity leaves the record unchanged with beam 1."""
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 8)
    out = rays.copy()
    beam = np.ones(rays.shape[0], dtype=F)
    if observer is None or observer.at_rest:
        return out, beam
    b = np.array([F(v) for v in observer.velocity], dtype=F)
    bb = F(F(F(b[0] * b[0]) + F(b[1] * b[1])) + F(b[2] * b[2]))
    if not np.all(np.isfinite(b)) or bb > F(0.9801):
        raise ValueError(f"boost_rays: the velocity {tuple(observer.velocity)} is not finite or faster than 0.99 c")
    ig = np.sqrt(F(F(1.0) - bb), dtype=F)
    g = F(F(1.0) / ig)
    k = F(g / F(g + F(1.0)))
    n = rays[:, 4:7]
    live = ~np.all(n == F(0.0), axis=1)
    with np.errstate(all="ignore"):
        c = _dot(b[None, :], n).astype(F)
        a = ((k * c).astype(F) - F(1.0)).astype(F)
        q = (F(1.0) / (F(1.0) - c).astype(F)).astype(F)
        v = ((((n * ig).astype(F) + (b[None, :] * a[:, None]).astype(F)).astype(F)) * q[:, None]).astype(F)
        d = _normalize(v)
        D = (ig * q).astype(F)
        D2 = (D * D).astype(F)
        B = (D2 * D2).astype(F)
    out[live, 4:7] = d[live]
    beam[live] = B[live]
    return out, beam
