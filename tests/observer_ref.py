"""The moving observer of stills (bhray_accum_set_observer) restated in NumPy from include/bhray.h's contract, binary32 operation by operation: the
Lorentz aberration of a rest-frame look direction and the beam D^4, over the records of tests/still_camera_ref.sample_rays.  Written from the contract, not from
bhusie_amd/cameras.boost_rays, with which it shares no function.  Also the binary64 formula the rule is measured against.  What tests/test_observer_cpu.py,
tests/test_observer_host.py and tests/test_gpu_observer.py compare with."""
from __future__ import annotations

import numpy as np

from tests import still_camera_ref as SR

f = np.float32
MAX_SPEED2 = f(0.9801)


def _m(a, b):
    return np.multiply(a, b, dtype=f)


def _a(a, b):
    return np.add(a, b, dtype=f)


def _s(a, b):
    return np.subtract(a, b, dtype=f)


def _d(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.divide(a, b, dtype=f)


def speed2(velocity):
    b = np.asarray(velocity, dtype=f)
    return _a(_a(_m(b[0], b[0]), _m(b[1], b[1])), _m(b[2], b[2]))


def at_rest(velocity) -> bool:
    return velocity is None or bool((np.asarray(velocity, dtype=f) == f(0.0)).all())


def constants(velocity):
    """(b, ig, k): once per call"""
    b = np.asarray(velocity, dtype=f)
    ig = np.sqrt(_s(f(1.0), speed2(b)), dtype=f)
    g = _d(f(1.0), ig)
    return b, ig, _d(g, _a(g, f(1.0)))


def boost(directions, velocity):
    """(n, beam) of the (m, 3) binary32 rest-frame directions n' under `velocity`: the per-record rule.  An all-zero n' passes unchanged with beam 1; a velocity that
    is None or all zero changes nothing."""
    n = np.ascontiguousarray(directions, dtype=f).reshape(-1, 3)
    out, beam = n.copy(), np.ones(n.shape[0], dtype=f)
    if at_rest(velocity):
        return out, beam
    b, ig, k = constants(velocity)
    with np.errstate(all="ignore"):
        c = _a(_a(_m(b[0], n[:, 0]), _m(b[1], n[:, 1])), _m(b[2], n[:, 2]))
        a = _s(_m(k, c), f(1.0))
        q = _d(f(1.0), _s(f(1.0), c))
        v = np.stack([_m(_a(_m(n[:, i], ig), _m(b[i], a)), q) for i in range(3)], axis=1)
        r = _d(f(1.0), np.sqrt(_a(_a(_m(v[:, 0], v[:, 0]), _m(v[:, 1], v[:, 1])), _m(v[:, 2], v[:, 2])), dtype=f))
        d = _m(v, r[:, None])
        D = _m(ig, q)
        D2 = _m(D, D)
        B = _m(D2, D2)
    live = (n != f(0.0)).any(axis=1)
    out[live], beam[live] = d[live], B[live]
    return out, beam


def boost_rays(rays, velocity):
    """(rays', beam): (m, 8) records with their directions boosted, origins and pads untouched"""
    rays = np.ascontiguousarray(rays, dtype=f).reshape(-1, 8)
    out = rays.copy()
    out[:, 4:7], beam = boost(rays[:, 4:7], velocity)
    return out, beam


def sample_rays(camera_uniform: bytes, cfg, still, velocity, s: int):
    """(records, beam) of sample s under the still camera `still` (a still_camera_ref.Still or None) seen by the observer"""
    return boost_rays(SR.sample_rays(camera_uniform, cfg, still, s), velocity)


def exact(directions, velocity):
    """(n, D) by the binary64 formula n = (n'/gamma + b (gamma/(gamma+1) b.n' - 1)) / (1 - b.n'), D = 1 / (gamma (1 - b.n')), for unit n' (normalised here in binary64)"""
    n = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    b = np.asarray(velocity, dtype=np.float64)
    gamma = 1.0 / np.sqrt(1.0 - b @ b)
    c = n @ b
    v = (n / gamma + b[None, :] * (gamma / (gamma + 1.0) * c - 1.0)[:, None]) / (1.0 - c)[:, None]
    return v, 1.0 / (gamma * (1.0 - c))
