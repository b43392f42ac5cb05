"""CPU: the accumulation image's entry points (bhray_accum_*) exist in the headers, the library and every binding; the refusals that need no device; the
hosts carry the feature; the C++ program's --spp fails loudly without a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import bhusie_amd as B
from bhusie_amd import cameras, layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PRODUCT = {"bhray_accum_begin": 1, "bhray_accum_add": 2, "bhray_accum_samples": 2, "bhray_accum_read": 3, "bhray_accum_read_display": 3, "bhray_accum_sample_offset": 3}
DIAG = {"bhray_accum_sample_rays": 3, "bhray_accum_set_launch_rays": 2}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr, diag = _header("bhray.h"), _header("bhray_diag.h")
    for names, text, table in ((PRODUCT, hdr, layouts.SYMBOLS), (DIAG, diag, layouts.DIAG_SYMBOLS)):
        for name, nargs in names.items():
            assert re.search(r"\b(int|void) %s\s*\(" % name, text), f"{name} is not declared"
            assert name in table and len(table[name][1]) == nargs, name
            assert len(getattr(L, name).argtypes) == nargs      # AttributeError: not exported
    for name in DIAG:
        assert not re.search(r"\b%s\b" % name, hdr), f"{name} belongs to bhray_diag.h"
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"
    assert re.search(r"#define BHRAY_ACCUM_MAX_SAMPLES 65536u", hdr) and layouts.ACCUM_MAX_SAMPLES == 65536


def test_a_null_ctx_or_output_is_refused_without_a_device():
    L = B.lib()
    n = C.c_uint32(7)
    buf = (C.c_float * 16)()
    assert L.bhray_accum_begin(None) == E_INVALID
    assert L.bhray_accum_add(None, 4) == E_INVALID
    assert L.bhray_accum_add(None, 0) == E_INVALID
    assert L.bhray_accum_samples(None, C.byref(n)) == E_INVALID and n.value == 7
    assert L.bhray_accum_read(None, buf, 64) == E_INVALID
    assert L.bhray_accum_read_display(None, buf, 16) == E_INVALID
    assert L.bhray_accum_sample_rays(None, 0, None) == E_INVALID
    assert L.bhray_accum_set_launch_rays(None, 0) == E_INVALID


def test_the_hosts_carry_the_feature():
    for m in ("accum_begin", "accum_add", "accum_samples", "accum_read", "accum_read_display", "accum_sample_rays", "accum_set_launch_rays"):
        assert hasattr(B.RayPass, m), m
    sig = inspect.signature(B.Renderer.render_still)
    assert sig.parameters["samples"].default == 16 and sig.parameters["shutter"].default == 0.0
    assert inspect.signature(B.Renderer.save_still).parameters["samples"].default == 16
    p = inspect.signature(cameras.pinhole_rays).parameters
    assert p["offset"].default == (0.0, 0.0) and p["level"].default is None and p["crop"].default == (0, 0)
    assert callable(cameras.r2_offset)
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert re.search(r"std::vector<float> accumulate\(uint32_t samples\)", hpp) and "bhray_accum_add(" in hpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_accum.hip" in mk and "bhray_accum.o" in mk and "bhray_accum.h" in mk and "bhray_tex.h" in mk
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 18\. ", design, flags=re.M)


def test_render_still_refuses_a_bad_sample_count_before_any_call():
    r = B.Renderer.__new__(B.Renderer)                           # no ctx: the argument check comes first
    for bad in (0, -3):
        try:
            B.Renderer.render_still(r, samples=bad)
        except ValueError as e:
            assert "samples" in str(e)
        else:
            raise AssertionError("render_still accepted samples = %d" % bad)


def test_the_spp_program_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--spp" in src and "render_still" in src
    for bad_args in (["--spp"], ["--spp", "0"], ["--spp", "65537"], ["--spp", "4", "--panorama", "8", "4"]):
        bad = subprocess.run([exe, str(tmp_path / "o.f32")] + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and not (tmp_path / "o.f32").exists(), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_accum.py runs the program
    r = subprocess.run([exe, str(tmp_path / "o.f32"), "--base", "24", "14", "--levels", "1", "--spp", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stderr.strip(), "no GPU: the program must say so and fail"
    assert not (tmp_path / "o.f32").exists()
