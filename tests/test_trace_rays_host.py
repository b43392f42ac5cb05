"""CPU: the ray-batch entry points (bhray_trace_rays, bhray_trace_rays_device, bhray_trace_rays_sky) exist, are bound, refuse a NULL ctx without a
device, and bhray_ray has the layout the kernel loads; the seeded ray list of tests/test_gpu_trace_rays.py holds every outcome, by the oracle."""
import ctypes as C
import os
import re

import numpy as np

import bhusie_amd as B
from bhusie_amd import layouts
from tests import rays_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("bhray_trace_rays", "bhray_trace_rays_device", "bhray_trace_rays_sky")


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bhray.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), f"{name} is not declared in include/bhray.h"
        assert name in layouts.SYMBOLS, f"{name} is not in layouts.SYMBOLS"
        f = getattr(L, name)                                     # AttributeError: not exported
        assert f.restype is C.c_int and len(f.argtypes) == len(layouts.SYMBOLS[name][1])
    assert [len(layouts.SYMBOLS[n][1]) for n in NAMES] == [4, 5, 5]
    assert re.search(r"#define BHRAY_MAX_RAYS_PER_CALL \(1u << 26\)", hdr) and layouts.MAX_RAYS_PER_CALL == 1 << 26
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr)
    assert hasattr(B.RayPass, "trace_rays") and hasattr(B.RayPass, "trace_rays_device") and hasattr(B.Renderer, "render_rays")


def test_bhray_ray_is_two_16_byte_halves():
    R = layouts.BhrayRay
    assert C.sizeof(R) == 32
    assert (R.origin.offset, R.pad0.offset, R.direction.offset, R.pad1.offset) == (0, 12, 16, 28)
    assert B.BhrayRay is R
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_ray, 32)" in src and "OFF(bhray_ray, direction, 16)" in src
    rec = B.RayPass._ray_records(np.arange(12, dtype=np.float32).reshape(2, 6))       # (n, 6) -> records
    assert rec.shape == (2, 8) and rec[1].tolist() == [6.0, 7.0, 8.0, 0.0, 9.0, 10.0, 11.0, 0.0]


def test_a_null_ctx_is_refused_without_a_device():
    L = B.lib()
    rays = (layouts.BhrayRay * 4)()
    out = (C.c_float * 16)()
    assert L.bhray_trace_rays(None, rays, 4, out) == E_INVALID
    assert L.bhray_trace_rays(None, None, 0, None) == E_INVALID
    assert L.bhray_trace_rays_device(None, None, 4, None, None) == E_INVALID
    assert L.bhray_trace_rays_sky(None, rays, 4, out, None) == E_INVALID


def test_the_seeded_rays_hold_every_outcome_by_the_oracle():
    """the precondition of the GPU comparison, on the CPU: at least 300 rays each with a disk contribution, into the horizon, and escaping from either side of the sphere"""
    rec = RR.seeded_rays()
    assert rec.shape == (4133, 8) and rec.shape[0] % 64 != 0
    d = np.linalg.norm(rec[:, 0:3].astype(np.float64), axis=1)
    assert 3.0 <= d.min() and d.max() <= 60.0
    inside = d < RR.R_SPHERE
    assert inside[0::2].all() and not inside[1::2].any()          # alternating by index: every wave starts in both modes
    n2 = (rec[:, 4:7].astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(n2 - 1.0).max() < 3e-7
    for method in (0, 1):
        counts = RR.class_counts(*RR.reference(method))
        assert min(counts.values()) >= RR.MIN_PER_CLASS, counts
    counts = RR.class_counts(*RR.reference(1, True))
    assert min(counts.values()) >= RR.MIN_PER_CLASS, counts
    assert int((RR.reference(1, False)[1] != RR.reference(1, True)[1]).any(axis=1).sum()) >= 20
