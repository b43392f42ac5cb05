"""CPU: the surface of the still passes (bhray_accum_set_passes) without a device: the entry points in the header, the library and every binding;
the constants; the refusals that need no ctx (the ctx's own run in tests/test_gpu_accum_passes.py); the hosts and the documents; bhray_render's new argument."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import bhusie_amd as B
from bhusie_amd import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = {"bhray_accum_set_passes": 2, "bhray_accum_passes": 2, "bhray_accum_read_pass": 4, "bhray_accum_pass_values": 6}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr, diag = _header("bhray.h"), _header("bhray_diag.h")
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, f"{name} is not declared in bhray.h"
        assert m.group(1).count(",") + 1 == nargs == len(layouts.SYMBOLS[name][1]), name
        assert layouts.SYMBOLS[name][0] is C.c_int and name not in layouts.DIAG_SYMBOLS and not re.search(r"\b%s\b" % name, diag)
        assert len(getattr(L, name).argtypes) == nargs           # AttributeError: not exported
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"


def test_the_constants():
    hdr = _header("bhray.h")
    for name, value in (("COVERAGE", 1), ("GEOMETRY", 2), ("POSITION", 4), ("ESCAPE", 8)):
        m = re.search(r"BHRAY_PASS_%s\s*=\s*1u\s*<<\s*(\d)" % name, hdr)
        assert m and 1 << int(m.group(1)) == value == getattr(layouts, "PASS_" + name) == getattr(B, "PASS_" + name), name
        assert layouts.PASS_NAMES[name.lower()] == value
    assert re.search(r"BHRAY_PASS_ALL\s*=\s*0xfu", hdr) and layouts.PASS_ALL == B.PASS_ALL == 0xF
    assert sorted(layouts.PASS_NAMES) == ["coverage", "escape", "geometry", "position"]


def test_refusals_that_need_no_ctx():
    L = B.lib()
    word = C.c_uint32(77)
    for passes in (0, 1, layouts.PASS_ALL, 0x10, 0xFFFFFFFF):
        assert L.bhray_accum_set_passes(None, passes) == E_INVALID, "a NULL ctx"
    assert L.bhray_accum_passes(None, C.byref(word)) == E_INVALID and word.value == 77
    buf = np.zeros(16, np.float32)
    assert L.bhray_accum_read_pass(None, 1, buf.ctypes.data, 16) == E_INVALID
    # bhray_accum_pass_values: exactly one pass bit, and the arrays that pass reads
    n = 3
    r, q, d, out = np.zeros((n, 4), np.float32), np.zeros(n, B.RAY_RECORD_DTYPE), np.zeros((n, 8), np.float32), np.full((n, 4), 7.0, np.float32)
    args = (r.ctypes.data, q.ctypes.data, d.ctypes.data)
    for bad in (0, 3, 5, 0xF, 0x10, 0x18, 0xFFFFFFFF):
        assert L.bhray_accum_pass_values(*args, n, bad, out.ctypes.data) == E_INVALID, hex(bad)
    assert (out == 7.0).all(), "a refused call touched the output"
    for bit in (1, 2, 4, 8):
        assert L.bhray_accum_pass_values(None, q.ctypes.data, d.ctypes.data, n, bit, out.ctypes.data) == E_INVALID
        assert L.bhray_accum_pass_values(r.ctypes.data, None, d.ctypes.data, n, bit, out.ctypes.data) == E_INVALID
        assert L.bhray_accum_pass_values(*args, n, bit, None) == E_INVALID
        assert L.bhray_accum_pass_values(r.ctypes.data, q.ctypes.data, None, n, bit, out.ctypes.data) == (E_INVALID if bit == 8 else 0), "rays may be NULL except for ESCAPE"
        assert L.bhray_accum_pass_values(None, None, None, 0, bit, None) == 0, "n == 0 reads nothing"
    try:
        B.accum_pass_values(r, q, None, layouts.PASS_ESCAPE)
        raise AssertionError("accum_pass_values took ESCAPE without rays")
    except B.BhrayError as e:
        assert e.code == E_INVALID
    try:
        B.accum_pass_values(r, q[:2], None, layouts.PASS_COVERAGE)
        raise AssertionError("accum_pass_values took arrays of different lengths")
    except ValueError:
        pass


def test_the_hosts_carry_the_feature():
    for name in ("accum_set_passes", "accum_passes", "accum_read_pass"):
        assert hasattr(B.RayPass, name), name
    assert inspect.signature(B.RayPass.accum_set_passes).parameters["passes"].default == 0
    assert list(inspect.signature(B.accum_pass_values).parameters) == ["results", "records", "rays", "pass_bit"]
    assert inspect.signature(B.Renderer.render_still).parameters["passes"].default == 0
    assert inspect.signature(B.Renderer.save_still).parameters["passes"].default == 0
    assert hasattr(B.Renderer, "still_pass")
    assert B.Renderer._pass_bits("coverage,escape") == 9 and B.Renderer._pass_bits(["geometry", 4]) == 6 and B.Renderer._pass_bits(0) == 0 and B.Renderer._pass_bits(None) == 0
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert re.search(r"^\s*uint32_t still_passes\b", hpp, flags=re.M) and re.search(r"std::vector<float> still_pass\(uint32_t", hpp)
    assert "bhray_accum_set_passes(" in hpp and "bhray_accum_read_pass(" in hpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_accum_passes.hip" in mk and "bhray_accum_passes.o" in mk and "bhray_accum_passes.h" in mk
    api = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_api.hip")).read()
    assert "launch_accum_passes_add(" in api and "launch_accum_passes_form(" in api
    kernels = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_accum_passes.hip")).read()
    for name in ("accum_passes_add_kernel", "accum_passes_form_kernel"):
        assert re.search(r"__global__[^\n]*\b%s\(" % name, kernels), name
    assert kernels.count("accum_pass_value(") >= 3, "the two kernels and the host form call one function"
    assert re.search(r"BH_HD bool accum_pass_value\(", open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_accum_passes.h")).read())
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 27\. ", design, flags=re.M) and "bhray_accum_set_passes" in design and "list form" in design
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in md, name
    assert "BHRAY_PASS_ALL" in md
    assert "bhray_accum_set_passes" in open(os.path.join(ROOT, "README.md")).read()


def test_the_programs_arguments(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--passes" in src
    out = str(tmp_path / "o.f32")
    small = ["--base", "24", "14", "--levels", "1"]
    for bad_args in (["--passes", "coverage"], ["--spp", "2", "--passes"], ["--spp", "2", "--passes", "depth"], ["--spp", "2", "--passes", "coverage,,escape"],
                     ["--spp", "2", "--passes", ""], ["--spp-adaptive", "2", "6", "0.05", "--spp-round", "2", "--passes", "coverage"],
                     ["--panorama", "8", "4", "--passes", "escape"], ["--spp", "2", "--panorama", "8", "4", "--passes", "escape"]):
        bad = subprocess.run([exe, out] + small + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and bad.stderr.strip() and not os.path.exists(out), bad_args
        assert not any(os.path.exists(out + "." + name) for name in layouts.PASS_NAMES), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_accum_passes.py runs the program
    for good in (["--spp", "2", "--passes", "coverage"], ["--spp", "2", "--passes", "coverage,geometry,position,escape"],
                 ["--spp", "2", "--filter", "tent", "1.5", "--passes", "escape,coverage"]):
        r = subprocess.run([exe, out] + small + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (good, r.returncode, r.stderr)   # parsed and accepted: it fails at the device, not at the arguments
