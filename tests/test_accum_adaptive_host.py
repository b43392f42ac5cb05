"""CPU: the entry points of adaptive stills (bhray_accum_add_adaptive) exist in the headers, the library and every binding, with the structs' layouts;
the refusals that need no device; the hosts carry the feature; the C++ program's --spp-adaptive argument errors."""
import ctypes as C
import inspect
import os
import re
import subprocess

import bhusie_amd as B
from bhusie_amd import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PRODUCT = {"bhray_accum_add_adaptive": 3, "bhray_accum_read_counts": 3}
DIAG = {"bhray_accum_active_pixels": 5}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _struct(text, name):
    """[(ctype, field)] of `typedef struct name { ... } name;`"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    return [tuple(d.split()) for d in body.split(";") if d.strip()]


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr, diag = _header("bhray.h"), _header("bhray_diag.h")
    for names, text, table in ((PRODUCT, hdr, layouts.SYMBOLS), (DIAG, diag, layouts.DIAG_SYMBOLS)):
        for name, nargs in names.items():
            assert re.search(r"\bint %s\s*\(" % name, text), f"{name} is not declared"
            assert name in table and len(table[name][1]) == nargs, name
            assert len(getattr(L, name).argtypes) == nargs      # AttributeError: not exported
    for name in DIAG:
        assert not re.search(r"\b%s\b" % name, hdr), f"{name} belongs to bhray_diag.h"
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"


def test_the_structs_are_the_headers():
    hdr = _header("bhray.h")
    cmap = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for name, cls, size in (("bhray_accum_adaptive", layouts.BhrayAccumAdaptive, 24), ("bhray_accum_adaptive_info", layouts.BhrayAccumAdaptiveInfo, 24)):
        assert [(cmap[t], f) for t, f in _struct(hdr, name)] == [(t, f) for f, t in cls._fields_], name
        assert C.sizeof(cls) == size, name
    assert layouts.BhrayAccumAdaptive.tolerance.offset == 16 and layouts.BhrayAccumAdaptiveInfo.rays.offset == 8 and layouts.BhrayAccumAdaptiveInfo.reach.offset == 16
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "bhray_accum_adaptive_info" in src and "bhray_accum_adaptive," in src, "the layouts are static_assert-ed in the library"


def test_a_null_ctx_or_null_params_is_refused_without_a_device():
    L = B.lib()
    a = layouts.BhrayAccumAdaptive(C.sizeof(layouts.BhrayAccumAdaptive), 4, 12, 4, 0.05, 0.01)
    info = layouts.BhrayAccumAdaptiveInfo(rounds=7)
    n = C.c_uint32(7)
    buf = (C.c_uint32 * 16)()
    assert L.bhray_accum_add_adaptive(None, C.byref(a), C.byref(info)) == E_INVALID and info.rounds == 7
    assert L.bhray_accum_add_adaptive(None, None, None) == E_INVALID
    assert L.bhray_accum_read_counts(None, buf, 16) == E_INVALID
    assert L.bhray_accum_active_pixels(None, C.byref(a), buf, 16, C.byref(n)) == E_INVALID and n.value == 7
    assert L.bhray_accum_active_pixels(None, None, None, 0, None) == E_INVALID


def test_the_hosts_carry_the_feature():
    for m in ("accum_add_adaptive", "accum_read_counts", "accum_active_pixels"):
        assert hasattr(B.RayPass, m), m
    sig = inspect.signature(B.RayPass.accum_add_adaptive)
    assert list(sig.parameters)[1:] == ["min_samples", "max_samples", "round_samples", "tolerance", "dark"]
    still = inspect.signature(B.Renderer.render_still).parameters
    assert still["adaptive"].default is None and still["samples"].default == 16 and still["shutter"].default == 0.0, "the defaults are today's still"
    assert callable(B.Renderer.still_counts)
    p = B.AdaptiveStill(min_samples=4, max_samples=12, round_samples=4, tolerance=0.05, dark=0.0)
    assert p.as_kwargs() == {"min_samples": 4, "max_samples": 12, "round_samples": 4, "tolerance": 0.05, "dark": 0.0}
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert re.search(r"std::vector<float> accumulate_adaptive\(", hpp) and re.search(r"std::vector<float> render_still_adaptive\(", hpp) and "bhray_accum_add_adaptive(" in hpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_adapt.hip" in mk and "bhray_adapt.o" in mk and "bhray_adapt.h" in mk
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 20\. ", design, flags=re.M)


def test_an_adaptive_still_has_no_shutter():
    r = B.Renderer.__new__(B.Renderer)                           # no ctx: the argument check comes first
    try:
        B.Renderer.render_still(r, shutter=1.0, adaptive=B.AdaptiveStill())
    except ValueError as e:
        assert "shutter" in str(e)
    else:
        raise AssertionError("render_still accepted a shutter with an adaptive still")


def test_the_spp_adaptive_argument_errors(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--spp-adaptive" in src and "render_still_adaptive" in src
    for bad_args in (["--spp-adaptive"], ["--spp-adaptive", "4", "12"], ["--spp-adaptive", "1", "9", "0.05"], ["--spp-adaptive", "8", "4", "0.05"],
                     ["--spp-adaptive", "4", "65540", "0.05"], ["--spp-adaptive", "4", "12", "-1"], ["--spp-adaptive", "4", "12", "nan"],
                     ["--spp-adaptive", "4", "13", "0.05"], ["--spp-adaptive", "4", "12", "0.05", "--spp-round", "0"], ["--spp-adaptive", "4", "12", "0.05", "--spp-round", "3"],
                     ["--spp-adaptive", "4", "12", "0.05", "--spp-dark", "-0.5"], ["--spp-adaptive", "4", "12", "0.05", "--spp-dark", "inf"],
                     ["--spp-adaptive", "4", "12", "0.05", "--spp", "4"], ["--spp", "4", "--spp-adaptive", "4", "12", "0.05"],
                     ["--spp-adaptive", "4", "12", "0.05", "--panorama", "8", "4"]):
        bad = subprocess.run([exe, str(tmp_path / "o.f32")] + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and bad.stderr.strip() and not (tmp_path / "o.f32").exists(), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_accum_adaptive.py runs the program
    r = subprocess.run([exe, str(tmp_path / "o.f32"), "--base", "24", "14", "--levels", "1", "--spp-adaptive", "4", "12", "0.05"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stderr.strip(), "no GPU: the program must say so and fail"
    assert not (tmp_path / "o.f32").exists()
