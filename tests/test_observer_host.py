"""CPU: the surface of the moving observer (bhray_accum_set_observer) without a device: the entry points in the headers, the library and every
binding; the struct's layout; the refusals that need no device (the ctx's own, "the observer in force untouched", run in tests/test_gpu_observer.py); the hosts and
the documents; bhray_render's new arguments."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import bhusie_amd as B
from bhusie_amd import cameras, layouts
from bhusie_amd.cameras import Observer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr, diag = _header("bhray.h"), _header("bhray_diag.h")
    for names, text, table in (({"bhray_accum_set_observer": 2, "bhray_observer_default": 1, "bhray_observer_boost_rays": 5}, hdr, layouts.SYMBOLS),
                               ({"bhray_observer_sample_rays_host": 7}, diag, layouts.DIAG_SYMBOLS)):
        for name, nargs in names.items():
            assert re.search(r"\b(int|void)\s+%s\s*\(" % name, text), f"{name} is not declared"
            assert name in table and len(table[name][1]) == nargs, name
            assert len(getattr(L, name).argtypes) == nargs      # AttributeError: not exported
    assert not re.search(r"\bbhray_observer_sample_rays_host\b", hdr), "the host form of the records belongs to bhray_diag.h"
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"
    assert re.search(r"#define BHRAY_OBSERVER_MAX_SPEED2 0\.9801f", hdr) and layouts.OBSERVER_MAX_SPEED2 == 0.9801


def test_the_struct_layout():
    S = layouts.BhrayObserver
    assert C.sizeof(S) == 20
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("struct_size", 0), ("velocity", 4), ("beaming", 16)]
    body = re.search(r"typedef struct bhray_observer \{(.*?)\} bhray_observer;", _header("bhray.h"), flags=re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+([a-z_]+)(?:\[3\])?;", body) == [("uint32_t", "struct_size"), ("float", "velocity"), ("uint32_t", "beaming")]
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_observer, 20)" in src and "OFF(bhray_observer, beaming, 16)" in src
    s = Observer((0.25, -0.5, 0.125), beaming=False).struct()
    assert (s.struct_size, tuple(s.velocity), s.beaming) == (20, (0.25, -0.5, 0.125), 0)
    assert Observer((0.1, 0.0, 0.0)).struct().beaming == 1 and not Observer((0.1, 0.0, 0.0)).at_rest and Observer((0.0, -0.0, 0.0)).at_rest


def test_refusals_that_need_no_device():
    L = B.lib()
    cfg = B.ladder_from_base((37, 33), 3, 1)
    cam = B.Camera().uniform()
    n = 37 * 33
    rays, beam = np.zeros((n, 8), np.float32), np.zeros(n, np.float32)
    rays[:, 6] = 1.0
    assert L.bhray_accum_set_observer(None, None) == E_INVALID
    L.bhray_observer_default(None)                                # no crash

    def both(velocity=(0.1, 0.0, 0.0), **kw):
        """the code of both host forms for the struct: they share the setter's validation"""
        s = Observer(velocity).struct()
        for k, v in kw.items():
            setattr(s, k, v)
        a = L.bhray_observer_sample_rays_host(C.byref(cfg), cam, None, C.byref(s), 0, rays.ctypes.data, beam.ctypes.data)
        b = L.bhray_observer_boost_rays(C.byref(s), rays.ctypes.data, n, rays.ctypes.data, None)
        assert a == b, (a, b)
        return a
    assert both() == 0
    assert both(struct_size=16) == E_INVALID and both(struct_size=24) == E_INVALID and both(struct_size=0) == E_INVALID
    for v in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, -float("inf"))):
        assert both(v) == E_INVALID, v
    assert both((0.995, 0.0, 0.0)) == E_INVALID and both((0.7, 0.7, 0.1)) == E_INVALID and both((0.0, 0.0, -1.0)) == E_INVALID
    assert both((0.98, 0.0, 0.0)) == 0 and both((0.0, -0.7, 0.7)) == 0, "bb = 0.98 <= 0.9801"
    assert both(beaming=2) == E_INVALID and both(beaming=0) == 0
    assert both((0.0, 0.0, 0.0), beaming=2) == E_INVALID, "beaming is checked whatever the velocity"
    s = Observer((0.1, 0.0, 0.0)).struct()
    assert L.bhray_observer_boost_rays(C.byref(s), None, 4, rays.ctypes.data, None) == E_INVALID
    assert L.bhray_observer_boost_rays(C.byref(s), rays.ctypes.data, 4, None, None) == E_INVALID
    p = rays.ctypes.data
    assert L.bhray_observer_sample_rays_host(None, cam, None, C.byref(s), 0, p, None) == E_INVALID
    assert L.bhray_observer_sample_rays_host(C.byref(cfg), None, None, C.byref(s), 0, p, None) == E_INVALID
    assert L.bhray_observer_sample_rays_host(C.byref(cfg), cam, None, C.byref(s), 0, None, None) == E_INVALID
    assert L.bhray_observer_sample_rays_host(C.byref(cfg), cam, None, C.byref(s), 65536, p, None) == E_INVALID
    assert L.bhray_observer_sample_rays_host(C.byref(cfg), cam, None, None, 65536, p, None) == E_INVALID
    bad_cam = cameras.StillCamera.fisheye(7.0).struct()
    assert L.bhray_observer_sample_rays_host(C.byref(cfg), cam, C.byref(bad_cam), C.byref(s), 0, p, None) == E_INVALID
    try:
        cameras.boost_rays(rays, Observer((0.995, 0.0, 0.0)))
        raise AssertionError("cameras.boost_rays took 0.995 c")
    except ValueError:
        pass


def test_the_hosts_carry_the_feature():
    assert hasattr(B.RayPass, "accum_set_observer") and B.Observer is Observer
    sig = inspect.signature(B.RayPass.accum_set_observer).parameters
    assert sig["velocity"].default is None and sig["beaming"].default is True
    assert inspect.signature(B.Renderer.render_still).parameters["observer"].default is None
    assert inspect.signature(B.Renderer.save_still).parameters["observer"].default is None
    assert list(inspect.signature(cameras.boost_rays).parameters) == ["rays", "observer"]
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert re.search(r"^\s*bhray_observer observer\{", hpp, flags=re.M) and "bhray_accum_set_observer(" in hpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_observer.hip" in mk and "bhray_observer.o" in mk and "bhray_observer.h" in mk
    api = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_api.hip")).read()
    for name in ("launch_observer_gen(", "launch_observer_gen_list(", "launch_observer_beam(", "launch_observer_beam_list("):
        assert name in api, name
    kernels = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_observer.hip")).read()
    for name in ("observer_gen_kernel", "observer_gen_list_kernel", "observer_beam_kernel", "observer_beam_list_kernel"):
        assert re.search(r"__global__[^\n]*\b%s\(" % name, kernels), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 26\. ", design, flags=re.M) and "bhray_accum_set_observer" in design
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn bhray_accum_set_observer(" in md and "pub struct bhray_observer" in md
    assert "bhray_accum_set_observer" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "observer_cost.py"))


def test_the_programs_arguments(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--observer" in src and "--no-beaming" in src
    out = str(tmp_path / "o.f32")
    small = ["--base", "24", "14", "--levels", "1"]
    for bad_args in (["--spp", "2", "--observer"], ["--spp", "2", "--observer", "0.5", "0"], ["--observer", "0.5", "0", "0"], ["--spp", "2", "--observer", "1", "0", "0"],
                     ["--spp", "2", "--observer", "0.7", "0.7", "0.2"], ["--spp", "2", "--observer", "nan", "0", "0"], ["--spp", "2", "--observer", "inf", "0", "0"],
                     ["--spp", "2", "--no-beaming"], ["--observer", "0.5", "0", "0", "--panorama", "8", "4"]):
        bad = subprocess.run([exe, out] + small + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and bad.stderr.strip() and not os.path.exists(out), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_observer.py runs the program
    for good in (["--spp", "2", "--observer", "0.5", "0", "0"], ["--spp", "2", "--observer", "0", "-0.3", "0.2", "--no-beaming"],
                 ["--spp-adaptive", "2", "6", "0.05", "--spp-round", "2", "--observer", "0.5", "0", "0"], ["--spp", "2", "--still-camera", "equirect", "--observer", "0", "0", "0.98"]):
        r = subprocess.run([exe, out] + small + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (good, r.returncode, r.stderr)   # parsed and accepted: it fails at the device, not at the arguments
