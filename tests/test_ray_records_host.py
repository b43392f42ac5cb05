"""CPU: the ray-record entry points (bhray_trace_rays_records, bhray_trace_rays_records_device) exist, are bound, refuse a NULL ctx without a device; the
record's layout is the header's in every binding; the C++ host's --pick fails loudly without a GPU; the Rust declaration is there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bhusie_amd as B
from bhusie_amd import cameras, layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("bhray_trace_rays_records", "bhray_trace_rays_records_device")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bhray.h")).read(), flags=re.S)


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr = _header()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), f"{name} is not declared in include/bhray.h"
        assert name in layouts.SYMBOLS, f"{name} is not in layouts.SYMBOLS"
        f = getattr(L, name)                                     # AttributeError: not exported
        assert f.restype is C.c_int and len(f.argtypes) == len(layouts.SYMBOLS[name][1])
    assert [len(layouts.SYMBOLS[n][1]) for n in NAMES] == [5, 6]
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    for method in ("trace_rays_records", "trace_rays_records_device"):
        assert hasattr(B.RayPass, method)
    assert hasattr(B.Renderer, "pick") and hasattr(B.Renderer, "render_records")


def test_the_record_is_32_bytes_in_every_binding():
    R = layouts.BhrayRayRecord
    want = {"position": 0, "hit": 12, "triangle": 16, "iterations": 20, "closest": 24, "transmittance": 28}
    assert C.sizeof(R) == 32 and {n: getattr(R, n).offset for n in want} == want
    assert B.BhrayRayRecord is R
    dt = B.RAY_RECORD_DTYPE
    assert dt.itemsize == 32 and {n: dt.fields[n][1] for n in want} == want
    assert dt["position"].shape == (3,) and dt["hit"] == np.uint32 and dt["triangle"] == np.int32 and dt["iterations"] == np.uint32
    # the header's struct, member by member, and its static_assert block
    m = re.search(r"typedef struct bhray_ray_record \{(.*?)\} bhray_ray_record;", _header(), re.S)
    assert m, "bhray_ray_record is not declared in include/bhray.h"
    members = re.findall(r"(float|uint32_t|int32_t)\s+(\w+)(\[3\])?;", m.group(1))
    assert [(t, n, bool(a)) for t, n, a in members] == [("float", "position", True), ("uint32_t", "hit", False), ("int32_t", "triangle", False),
                                                       ("uint32_t", "iterations", False), ("float", "closest", False), ("float", "transmittance", False)]
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_ray_record, 32)" in src
    for name, off in want.items():
        assert f"OFF(bhray_ray_record, {name}, {off})" in src, name
    e = re.search(r"enum \{ BHRAY_HIT_NONE = 0, BHRAY_HIT_HORIZON = 1, BHRAY_HIT_DISK = 2, BHRAY_HIT_MESH = 3, BHRAY_HIT_UNUSABLE = 255 \};", _header())
    assert e and (B.HIT_NONE, B.HIT_HORIZON, B.HIT_DISK, B.HIT_MESH, B.HIT_UNUSABLE) == (0, 1, 2, 3, 255)


def test_a_null_ctx_is_refused_without_a_device():
    L = B.lib()
    rays = (layouts.BhrayRay * 4)()
    out = (C.c_float * 16)()
    recs = (layouts.BhrayRayRecord * 4)()
    assert L.bhray_trace_rays_records(None, rays, 4, out, recs) == E_INVALID
    assert L.bhray_trace_rays_records(None, None, 0, None, None) == E_INVALID
    assert L.bhray_trace_rays_records_device(None, None, 4, None, None, None) == E_INVALID


def test_one_pixels_pinhole_ray_is_the_whole_levels_row():
    """Renderer.pick forms its ray with cameras.pinhole_rays' arithmetic for the one pixel: the same bits as that row of the whole level"""
    cam = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
    w, h = 70, 40
    full = cameras.pinhole_rays(cam, w, h)
    for x, y in ((0, 0), (69, 39), (35, 20), (13, 31)):
        one = cameras.pinhole_rays(cam, w, h, pixel=(x, y))
        assert one.shape == (1, 8) and np.array_equal(one.view(np.uint32)[0], full.view(np.uint32)[y * w + x]), (x, y)


def test_the_pick_program_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--pick" in src and "Renderer::pick" in src
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert "trace_rays_records" in hpp and re.search(r"bhray_ray_record pick\(uint32_t x, uint32_t y\)", hpp)
    bad = subprocess.run([exe, str(tmp_path / "o.f32"), "--pick", "3"], capture_output=True, text=True, timeout=60)      # X without Y: the argument is refused
    assert bad.returncode == 2 and not (tmp_path / "o.f32").exists()
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_ray_records.py runs the program
    r = subprocess.run([exe, str(tmp_path / "o.f32"), "--base", "24", "14", "--levels", "1", "--pick", "3", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stderr.strip(), "no GPU: the program must say so and fail"
    assert "pick" not in r.stdout and not (tmp_path / "o.f32").exists()


def test_the_rust_declaration_is_present():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"pub fn bhray_trace_rays_records\(ctx: \*mut bhray_ctx, rays: \*const c_void, n: u32, out_rgba32f: \*mut f32, out_records: \*mut c_void\) -> c_int;", doc)
    assert re.search(r"pub fn bhray_trace_rays_records_device\(ctx: \*mut bhray_ctx, d_rays: \*const c_void, n: u32, d_out_rgba32f: \*mut c_void, d_records: \*mut c_void, "
                     r"hip_stream: \*mut c_void\) -> c_int;", doc)
    assert "bhray_ray_record" in doc
