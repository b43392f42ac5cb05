"""CPU: the still pixel filters (bhray_accum_set_filter) without a device.

  1. bhray_accum_filter_weights - the kernel's own weight function compiled for the host - equals the NumPy restatement (tests/accum_filter_ref.py) in every word
     for s = 0 .. 4095: TENT radius 0.5, 1, 2.5; CUBIC radius 1, 2, 2.5 with (B, C) = (1/3, 1/3), (1, 0), (0, 0.5).
  2. Known answers: at s = 0 TENT radius 1 and CUBIC (0, 0.5) radius 2 weigh exactly (0, 0, 1, 0, 0); the five taps of TENT radius 1 and of every CUBIC radius 2
     sum to 1 within 2e-6; taps +-3 weigh nothing, so adding them changes no sum.
  3. Every refusal of bhray_accum_set_filter that needs no device (the struct's validation is the one bhray_accum_filter_weights runs); the symbols, the struct's
     size and offsets, the hosts; bhray_render --filter's argument errors.
  4. The restatement on a synthetic 9 x 7 result image with one NaN texel and one infinite texel: neither reaches any sum, and a corner pixel's sum.w is the product
     of its one-sided tap sums."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import layouts
from bhusie_amd.renderer import StillFilter
from tests import accum_filter_ref as FR
from tests import accum_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
THIRD = 1.0 / 3.0
FILTERS = {"tent_0.5": FR.tent(0.5), "tent_1": FR.tent(1.0), "tent_2.5": FR.tent(2.5)}
for _r in (1.0, 2.0, 2.5):
    for _n, (_b, _c) in {"mitchell": (THIRD, THIRD), "bspline": (1.0, 0.0), "catmull_rom": (0.0, 0.5)}.items():
        FILTERS[f"cubic_{_r:g}_{_n}"] = FR.cubic(_r, _b, _c)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _struct(f):
    return layouts.BhrayStillFilter(C.sizeof(layouts.BhrayStillFilter), f.kind, f.radius, f.b, f.c)


def _lib_weights(st, s):
    wx, wy = np.full(5, np.nan, np.float32), np.full(5, np.nan, np.float32)
    rc = B.lib().bhray_accum_filter_weights(C.byref(st), int(s), wx.ctypes.data_as(C.POINTER(C.c_float)), wy.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, wx, wy


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


# ---- 1. the C text and the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILTERS))
def test_the_host_weights_are_the_restatements(name):
    f = FILTERS[name]
    st = _struct(f)
    rx, ry = FR.weights_table(f, np.arange(4096))
    wx, wy = np.empty_like(rx), np.empty_like(ry)
    for s in range(4096):
        rc, wx[s], wy[s] = _lib_weights(st, s)
        assert rc == 0
    differ = int((_bits(wx) != _bits(rx)).sum()) + int((_bits(wy) != _bits(ry)).sum())
    for s in (0, 1, 7, 4095):                                     # the vectorised offsets are tests/accum_ref.py's
        assert [float(v[0]) for v in FR.offsets([s])] == [float(v) for v in A.offset(s)]
    assert differ == 0, f"{name}: {differ} of {4096 * 10} weights differ from the restatement"


def test_the_python_value_delivers_the_library_weights():
    for filt, ref in ((StillFilter.tent(1.5), FR.tent(1.5)), (StillFilter.mitchell(), FR.cubic(2.0, THIRD, THIRD)), (StillFilter.bspline(2.5), FR.cubic(2.5, 1.0, 0.0)),
                      (StillFilter(), FR.Filter())):
        for s in (0, 1, 7, 4095):
            wx, wy = filt.weights(s)
            rx, ry = FR.weights(ref, s)
            assert np.array_equal(_bits(wx), _bits(rx)) and np.array_equal(_bits(wy), _bits(ry)), (filt, s)
    assert StillFilter.tent().radius == 1.0 and StillFilter.mitchell().radius == 2.0 and (StillFilter.bspline().b, StillFilter.bspline().c) == (1.0, 0.0)
    assert StillFilter().kind == layouts.FILTER_BOX


# ---- 2. known answers ---------------------------------------------------------------------------------
def test_known_answers():
    centre = np.array([0, 0, 1, 0, 0], np.float32)
    for f in (FR.tent(1.0), FR.cubic(2.0, 0.0, 0.5)):
        rc, wx, wy = _lib_weights(_struct(f), 0)
        assert rc == 0 and np.array_equal(_bits(wx), _bits(centre)) and np.array_equal(_bits(wy), _bits(centre)), f
        rx, ry = FR.weights(f, 0)
        assert np.array_equal(_bits(rx), _bits(centre)) and np.array_equal(_bits(ry), _bits(centre))
    worst = 0.0
    unit = [n for n, f in FILTERS.items() if (f.kind, f.radius) in ((FR.TENT, 1.0), (FR.CUBIC, 2.0))]
    assert len(unit) == 4
    for name in unit:
        st = _struct(FILTERS[name])
        for s in range(4096):
            _, wx, wy = _lib_weights(st, s)
            worst = max(worst, abs(float(wx.astype(np.float64).sum()) - 1.0), abs(float(wy.astype(np.float64).sum()) - 1.0))
    print(f"worst |sum of the five taps - 1|: {worst:.3g}")
    assert worst <= 2e-6
    for name, f in FILTERS.items():                               # taps +-3: weight 0 at every radius limit, so seven taps sum as five do
        for a, b in zip(FR.weights_table(f, np.arange(4096)), FR.weights_table(f, np.arange(4096), reach=3)):
            assert not b[:, 0].any() and not b[:, 6].any() and np.array_equal(_bits(a), _bits(b[:, 1:6])), name
            assert np.array_equal(a.astype(np.float64).sum(axis=1), b.astype(np.float64).sum(axis=1))


def test_seven_taps_change_no_sum_of_an_image():
    rng = np.random.default_rng(5)
    res = [np.concatenate([rng.random((63, 3), dtype=np.float32), np.ones((63, 1), np.float32)], axis=1) for _ in range(3)]
    for f in (FR.tent(2.5), FR.cubic(2.5, THIRD, THIRD)):
        five, seven = FR.accumulate(res, None, f, 9, 7, s0=11), FR.accumulate(res, None, f, 9, 7, s0=11, reach=3)
        assert np.array_equal(_bits(five), _bits(seven))


# ---- 3. refusals, symbols, layout, hosts --------------------------------------------------------------
def test_refusals_that_need_no_device():
    L = B.lib()
    assert L.bhray_accum_set_filter(None, None) == E_INVALID
    L.bhray_still_filter_default(None)                            # no crash
    d = layouts.BhrayStillFilter()
    L.bhray_still_filter_default(C.byref(d))
    assert (d.struct_size, d.kind) == (20, layouts.FILTER_BOX) and _lib_weights(d, 3)[0] == 0
    box = _lib_weights(d, 3)
    assert list(box[1]) == [0, 0, 1, 0, 0] and list(box[2]) == [0, 0, 1, 0, 0]
    w = np.zeros(5, np.float32)
    p = w.ctypes.data_as(C.POINTER(C.c_float))
    ok = _struct(FR.tent(1.0))
    assert L.bhray_accum_filter_weights(None, 0, p, p) == E_INVALID
    assert L.bhray_accum_filter_weights(C.byref(ok), 0, None, p) == E_INVALID and L.bhray_accum_filter_weights(C.byref(ok), 0, p, None) == E_INVALID

    def bad(**kw):
        s = _struct(FR.cubic(2.0, THIRD, THIRD))
        for k, v in kw.items():
            setattr(s, k, v)
        return _lib_weights(s, 1)[0]
    nan, inf = float("nan"), float("inf")
    assert bad() == 0
    assert bad(struct_size=16) == E_INVALID and bad(struct_size=24) == E_INVALID and bad(struct_size=0) == E_INVALID
    assert bad(kind=3) == E_INVALID and bad(kind=0xffffffff) == E_INVALID
    for r in (0.49, 2.51, 0.0, -1.0, nan, inf):
        assert bad(kind=1, radius=r) == E_INVALID, r
    for r in (0.99, 0.5, 2.51, 0.0, -2.0, nan, inf, -inf):
        assert bad(kind=2, radius=r) == E_INVALID, r
    for v in (-0.01, 1.01, nan, inf):
        assert bad(b=v) == E_INVALID and bad(c=v) == E_INVALID, v
    for r in (0.5, 1.0, 2.5):
        assert bad(kind=1, radius=r) == 0
    assert bad(kind=2, radius=1.0) == 0 and bad(kind=2, radius=2.5) == 0 and bad(b=0.0, c=1.0) == 0 and bad(b=1.0, c=0.0) == 0
    assert bad(kind=1, b=nan, c=inf) == 0, "b and c are read for the cubic only"
    assert bad(kind=0, radius=nan, b=nan, c=nan) == 0, "the box reads nothing"


def test_the_symbols_and_the_struct_layout():
    L = B.lib()
    hdr = _header("bhray.h")
    for name, nargs in {"bhray_accum_set_filter": 2, "bhray_still_filter_default": 1, "bhray_accum_filter_weights": 4}.items():
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, hdr), f"{name} is not declared"
        assert name in layouts.SYMBOLS and len(layouts.SYMBOLS[name][1]) == nargs, name
        assert len(getattr(L, name).argtypes) == nargs          # AttributeError: not exported
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"
    assert re.search(r"BHRAY_FILTER_BOX = 0, BHRAY_FILTER_TENT = 1, BHRAY_FILTER_CUBIC = 2", hdr)
    assert (layouts.FILTER_BOX, layouts.FILTER_TENT, layouts.FILTER_CUBIC) == (0, 1, 2) == (FR.BOX, FR.TENT, FR.CUBIC)
    S = layouts.BhrayStillFilter
    assert C.sizeof(S) == 20
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("struct_size", 0), ("kind", 4), ("radius", 8), ("b", 12), ("c", 16)]
    body = re.search(r"typedef struct bhray_still_filter \{(.*?)\} bhray_still_filter;", hdr, flags=re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+([a-z_, ]+);", body) == [("uint32_t", "struct_size"), ("uint32_t", "kind"), ("float", "radius"), ("float", "b, c")]
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_still_filter, 20)" in src and "OFF(bhray_still_filter, c, 16)" in src
    s = StillFilter.mitchell(1.5).struct()
    assert (s.struct_size, s.kind, s.radius) == (20, 2, 1.5) and s.b == np.float32(THIRD) == s.c


def test_the_hosts_carry_the_feature():
    assert hasattr(B.RayPass, "accum_set_filter") and B.StillFilter is StillFilter
    assert inspect.signature(B.RayPass.accum_set_filter).parameters["filter"].default is None
    assert inspect.signature(B.Renderer.render_still).parameters["filter"].default is None
    assert inspect.signature(B.Renderer.save_still).parameters["filter"].default is None
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert "void set_still_filter(const bhray_still_filter* filter)" in hpp and "bhray_accum_set_filter(" in hpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_accum_filter.hip" in mk and "bhray_accum_filter.o" in mk and "bhray_accum_filter.h" in mk
    group = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_group.hip")).read()
    assert "dev_accum_set_filter(p.dev, filter)" in group, "a multi-device ctx forwards the call as it does the camera"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 22\. ", design, flags=re.M) and "bhray_accum_set_filter" in design and "accum_filter_add_kernel" in design
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn bhray_accum_set_filter(" in md and "pub struct bhray_still_filter" in md
    assert "bhray_accum_set_filter" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "accum_filter_cost.py"))


def test_the_programs_arguments(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = str(tmp_path / "o.f32")
    small = ["--base", "24", "14", "--levels", "1"]
    for bad_args in (["--spp", "4", "--filter"], ["--spp", "4", "--filter", "gauss", "1"], ["--spp", "4", "--filter", "tent"], ["--spp", "4", "--filter", "tent", "0.4"],
                     ["--spp", "4", "--filter", "tent", "2.6"], ["--spp", "4", "--filter", "tent", "nan"], ["--spp", "4", "--filter", "cubic", "2"],
                     ["--spp", "4", "--filter", "cubic", "2", "0.3"], ["--spp", "4", "--filter", "cubic", "0.9", "0.3", "0.3"], ["--spp", "4", "--filter", "cubic", "2.6", "0.3", "0.3"],
                     ["--spp", "4", "--filter", "cubic", "2", "1.1", "0.3"], ["--spp", "4", "--filter", "cubic", "2", "0.3", "-0.1"], ["--spp", "4", "--filter", "cubic", "2", "nan", "0"],
                     ["--filter", "tent", "1"], ["--spp-adaptive", "2", "6", "0.05", "--spp-round", "2", "--filter", "tent", "1"],
                     ["--spp-adaptive", "2", "6", "0.05", "--spp-round", "2", "--filter", "cubic", "2", "0.3333333", "0.3333333"],
                     ["--spp", "4", "--filter", "tent", "1", "--panorama", "8", "4"]):
        bad = subprocess.run([exe, out] + small + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and bad.stderr.strip() and not os.path.exists(out), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_accum_filter.py runs the program
    for good in (["--spp", "4", "--filter", "tent", "1.5"], ["--spp", "4", "--filter", "cubic", "2", "0.3333333", "0.3333333"],
                 ["--spp", "4", "--still-camera", "equirect", "--filter", "cubic", "2.5", "1", "0"]):
        r = subprocess.run([exe, out] + small + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (good, r.returncode, r.stderr)   # parsed and accepted: it fails at the device, not at the arguments


# ---- 4. the restatement's sum on a synthetic image ----------------------------------------------------
@pytest.mark.parametrize("name", ["tent_1", "tent_2.5", "cubic_2_mitchell", "cubic_2.5_catmull_rom"])
def test_the_restated_sum_on_a_synthetic_image(name):
    f = FILTERS[name]
    W, H, S = 9, 7, 4
    rng = np.random.default_rng(22)
    res = [np.concatenate([rng.random((W * H, 3), dtype=np.float32), np.ones((W * H, 1), np.float32)], axis=1) for _ in range(S)]
    for r in res:                                                 # one NaN texel and one infinite texel in every sample's image, away from the corner's support
        r[3 * W + 4, 1] = np.nan
        r[5 * W + 6, 0] = np.inf
    total = FR.accumulate(res, None, f, W, H)
    assert np.isfinite(total).all(), "a NaN or an infinite texel reached a sum"
    # the same sums from images in which the two texels are absent: V built by hand as (0, 0, 0, 0) there - no resolve, no select
    want = np.zeros((H, W, 4), np.float32)
    for s, r in enumerate(res):
        V = r.reshape(H, W, 4).copy()
        V[3, 4] = V[5, 6] = 0.0
        wx, wy = FR.weights(f, s)
        want = (want + FR.stencil(V, wx, wy)).astype(np.float32)
    assert np.array_equal(_bits(total), _bits(want.reshape(-1, 4)))
    full = FR.accumulate([np.where(np.isfinite(r), r, np.float32(0.5)) for r in res], None, f, W, H)
    near = np.zeros((H, W), bool)
    near[1:6, 2:7] = True; near[3:7, 4:9] = True                  # the pixels within 2 of (4, 3) or (6, 5)
    changed = (_bits(full) != _bits(total)).any(axis=1).reshape(H, W)
    assert not (changed & ~near).any(), "a skipped texel changed a pixel outside its reach"
    assert changed[3, 4] and changed[5, 6]
    # a corner pixel: its weight is the product of its one-sided tap sums, sample by sample (the bar: the roundings of the three products and the five additions of
    # each factor, relative to the sum of the taps' magnitudes)
    got, ref, mag = 0.0, 0.0, 0.0
    for s in range(S):
        wx, wy = (w.astype(np.float64) for w in FR.weights(f, s))
        ref += wx[2:].sum() * wy[2:].sum()
        mag += np.abs(wx[2:]).sum() * np.abs(wy[2:]).sum()
    got = float(total[0, 3])
    print(f"{name}: corner weight {got!r}, product of the one-sided tap sums {ref!r}")
    assert abs(got - ref) <= 16 * 2.0 ** -24 * mag
    assert got < float(total[(H // 2) * W + 1, 3]), "an edge pixel away from the corner receives more weight than the corner"
