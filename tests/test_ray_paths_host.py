"""CPU: the ray-path entry points (bhray_trace_rays_paths, bhray_trace_rays_paths_device) exist, are bound, refuse a NULL ctx without a device; a path
point's layout is the header's in every binding; the ray Renderer.ray_path traces is pick's; the C++ host's --path fails loudly without a GPU; the Rust declaration
is there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bhusie_amd as B
from bhusie_amd import cameras, layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("bhray_trace_rays_paths", "bhray_trace_rays_paths_device")


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
    assert [len(layouts.SYMBOLS[n][1]) for n in NAMES] == [9, 10]
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"
    assert re.search(r"#define BHRAY_MAX_PATH_STRIDE_LOG2\s+16\b", hdr) and layouts.MAX_PATH_STRIDE_LOG2 == 16
    assert re.search(r"#define BHRAY_MAX_PATH_POINTS_PER_CALL \(1u << 24\)", hdr) and layouts.MAX_PATH_POINTS_PER_CALL == 1 << 24
    for method in ("trace_rays_paths", "trace_rays_paths_device"):
        assert hasattr(B.RayPass, method)
    assert hasattr(B.Renderer, "ray_path")


def test_a_path_point_is_16_bytes_in_every_binding():
    P = layouts.BhrayPathPoint
    want = {"position": 0, "iteration": 12}
    assert C.sizeof(P) == 16 and {n: getattr(P, n).offset for n in want} == want
    assert B.BhrayPathPoint is P and B.PATH_POINT_DTYPE is layouts.PATH_POINT_DTYPE
    dt = B.PATH_POINT_DTYPE
    assert dt.itemsize == 16 and {n: dt.fields[n][1] for n in want} == want
    assert dt["position"].shape == (3,) and dt["position"].base == np.float32 and dt["iteration"] == np.uint32
    m = re.search(r"typedef struct bhray_path_point \{(.*?)\} bhray_path_point;", _header(), re.S)
    assert m, "bhray_path_point is not declared in include/bhray.h"
    members = re.findall(r"(float|uint32_t|int32_t)\s+(\w+)(\[3\])?;", m.group(1))
    assert [(t, n, bool(a)) for t, n, a in members] == [("float", "position", True), ("uint32_t", "iteration", False)]
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_path_point, 16)" in src
    for name, off in want.items():
        assert f"OFF(bhray_path_point, {name}, {off})" in src, name


def test_a_null_ctx_is_refused_without_a_device():
    L = B.lib()
    rays = (layouts.BhrayRay * 4)()
    out = (C.c_float * 16)()
    recs = (layouts.BhrayRayRecord * 4)()
    pts = (layouts.BhrayPathPoint * 8)()
    cnt = (C.c_uint32 * 4)()
    assert L.bhray_trace_rays_paths(None, rays, 4, 0, 2, out, recs, pts, cnt) == E_INVALID
    assert L.bhray_trace_rays_paths(None, None, 0, 0, 2, None, None, None, None) == E_INVALID
    assert L.bhray_trace_rays_paths_device(None, None, 4, 0, 2, None, None, None, None, None) == E_INVALID


def test_ray_path_traces_picks_ray():
    """Renderer.ray_path forms its ray as Renderer.pick does - cameras.pinhole_rays(..., pixel=), whose bits tests/test_ray_records_host.py holds to the whole level's -
    and sizes its row from max_iterations"""
    import inspect
    src = inspect.getsource(B.Renderer.ray_path)
    assert "pinhole_rays(self.camera, fw, fh, pixel=(int(x), int(y)))" in src and "pinhole_rays(self.camera, fw, fh, pixel=(int(x), int(y)))" in inspect.getsource(B.Renderer.pick)
    assert "max_iterations" in src
    cam = B.Camera()
    one = cameras.pinhole_rays(cam, 24, 14, pixel=(5, 9))
    assert one.shape == (1, 8) and np.array_equal(one.view(np.uint32)[0], cameras.pinhole_rays(cam, 24, 14).view(np.uint32)[9 * 24 + 5])


def test_the_path_program_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--path" in src and "--path-stride" in src and "Renderer::ray_path" in src
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert "bhray_trace_rays_paths(" in hpp and re.search(r"RayPath ray_path\(uint32_t x, uint32_t y, uint32_t stride_log2 = 0\)", hpp)
    for bad_args in (["--path", "3"], ["--path", "3", "4", "--path-stride", "17"], ["--path", "3", "4", "--panorama", "8", "4"]):
        bad = subprocess.run([exe, str(tmp_path / "o.f32")] + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and not (tmp_path / "o.f32").exists(), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_ray_paths.py runs the program
    r = subprocess.run([exe, str(tmp_path / "o.f32"), "--base", "24", "14", "--levels", "1", "--path", "3", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stderr.strip(), "no GPU: the program must say so and fail"
    assert "pick" not in r.stdout and not (tmp_path / "o.f32").exists()


def test_the_rust_declaration_is_present():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"pub fn bhray_trace_rays_paths\(ctx: \*mut bhray_ctx, rays: \*const c_void, n: u32, stride_log2: u32, max_points: u32, out_rgba32f: \*mut f32, "
                     r"out_records: \*mut c_void, out_points: \*mut c_void, out_counts: \*mut u32\) -> c_int;", doc)
    assert re.search(r"pub fn bhray_trace_rays_paths_device\(ctx: \*mut bhray_ctx, d_rays: \*const c_void, n: u32, stride_log2: u32, max_points: u32, d_out_rgba32f: \*mut c_void, "
                     r"d_records: \*mut c_void, d_points: \*mut c_void, d_counts: \*mut c_void, hip_stream: \*mut c_void\) -> c_int;", doc)
    assert "bhray_path_point" in doc
