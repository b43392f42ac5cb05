"""CPU: the still cameras (bhray_accum_set_camera) without a device.

  1. bhray_still_sample_rays_host - the kernels' own function compiled for the host - equals the NumPy restatement (tests/still_camera_ref.py) in every word, and
     so does cameras.still_rays.
  2. With the default camera the host function is tests/accum_ref.sample_rays bit for bit.
  3. At sample 0 the equirect and fisheye restatements lie within 1e-6 per component of cameras.equirect_rays / fisheye_rays; the fisheye's masks are equal.
  4. The lens: origins on the aperture disk in the right / up plane, every ray through its point of focus, the disk covered evenly.
  5. The entry points exist in the headers, the library, every binding, renderer.hpp and DESIGN.md; the struct's layout; the refusals that need no device;
     bhray_render's new arguments."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras, layouts
from bhusie_amd.cameras import StillCamera
from tests import accum_ref as A
from tests import still_camera_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1)}
CAM = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
CAMERAS = {"pinhole": (StillCamera.pinhole(), SR.Still()),
           "equirect": (StillCamera.equirect(), SR.Still(SR.EQUIRECT)),
           "fisheye": (StillCamera.fisheye(3.4), SR.Still(SR.FISHEYE, fisheye_fov=3.4)),
           "lens": (StillCamera.pinhole(lens_radius=0.35, focus_distance=7.5), SR.Still(SR.PINHOLE, lens_radius=0.35, focus_distance=7.5))}
SAMPLES = (0, 1, 7, 65535)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(cfg, cam_bytes, still, s):
    out = np.empty((int(cfg.frame_w) * int(cfg.frame_h), 8), dtype=np.float32)
    st = still.struct() if still is not None else None
    rc = B.lib().bhray_still_sample_rays_host(C.byref(cfg), cam_bytes, C.byref(st) if st is not None else None, int(s), out.ctypes.data_as(C.POINTER(layouts.BhrayRay)))
    assert rc == 0, rc
    return out


# ---- 1. the C text, the restatement and the package's generator ---------------------------------------
@pytest.mark.parametrize("kind", list(CAMERAS))
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_host_function_is_the_restatement(shape, kind):
    cfg = CFGS[shape]()
    still, ref = CAMERAS[kind]
    for s in SAMPLES:
        want = SR.sample_rays(CAM.uniform(), cfg, ref, s)
        got = _host(cfg, CAM.uniform(), still, s)
        assert got.shape == want.shape
        differ = int((_bits(got) != _bits(want)).sum())
        assert differ == 0, f"{kind} sample {s}: {differ} of {got.size} words of the host function differ from the restatement"
        mine = cameras.still_rays(CAM, cfg, still, s)
        differ = int((_bits(mine) != _bits(want)).sum())
        assert differ == 0, f"{kind} sample {s}: {differ} of {got.size} words of cameras.still_rays differ from the restatement"
    if shape == "40x36_of_a_ladder":
        assert (cfg.crop_x, cfg.crop_y) != (0, 0) or (cfg.frame_w, cfg.frame_h) != tuple(cfg.sizes()[-1]), "the frame must be a window of its level"


@pytest.mark.parametrize("kind", list(CAMERAS))
def test_a_cropped_frame_is_a_window_of_the_whole_level(kind):
    cfg = CFGS["40x36_of_a_ladder"]()
    lw, lh = cfg.sizes()[-1]
    whole = B.ladder_from_base((lw, lh), 3, 1)
    still, _ = CAMERAS[kind]
    for s in (0, 7):
        level = _host(whole, CAM.uniform(), still, s).reshape(lh, lw, 8)
        window = level[cfg.crop_y:cfg.crop_y + cfg.frame_h, cfg.crop_x:cfg.crop_x + cfg.frame_w].reshape(-1, 8)
        assert np.array_equal(_bits(_host(cfg, CAM.uniform(), still, s)), _bits(window))


# ---- 2. the default camera ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_default_camera_is_the_pinhole_generator(shape):
    cfg = CFGS[shape]()
    for s in SAMPLES:
        want = A.sample_rays(CAM, cfg, s)
        assert np.array_equal(_bits(_host(cfg, CAM.uniform(), None, s)), _bits(want)), s
        assert np.array_equal(_bits(_host(cfg, CAM.uniform(), StillCamera(), s)), _bits(want)), s
        assert np.array_equal(_bits(cameras.still_rays(CAM, cfg, None, s)), _bits(want)), s
    d = layouts.BhrayStillCamera()
    B.lib().bhray_still_camera_default(C.byref(d))
    assert (d.struct_size, d.projection, d.lens_radius) == (20, 0, 0.0) and StillCamera().is_default


# ---- 3. against the pixel-centre generators -------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 32), (40, 37), (33, 32)])
def test_sample_0_lies_on_the_pixel_centre_generators(size):
    cfg = B.ladder_from_base(size, 3, 1)
    w, h = size
    u = np.frombuffer(CAM.uniform(), dtype=np.float32)
    pos, fwd = u[0:3], u[4:7]
    eq = SR.sample_rays(CAM.uniform(), cfg, SR.Still(SR.EQUIRECT), 0)
    want = cameras.equirect_rays(pos, fwd, w, h)
    err = float(np.abs(eq[:, 4:7].astype(np.float64) - want[:, 4:7]).max())
    print(f"equirect {w}x{h}: max component difference {err:.3g}")
    assert err <= 1e-6 and np.array_equal(eq[:, 0:4], want[:, 0:4])
    for fov in (3.4, 1.0, 2.0 * math.pi):
        fe = SR.sample_rays(CAM.uniform(), cfg, SR.Still(SR.FISHEYE, fisheye_fov=fov), 0)
        want = cameras.fisheye_rays(pos, fwd, w, h, fov)
        inside_got, inside_want = (fe[:, 4:7] != 0).any(axis=1), (want[:, 4:7] != 0).any(axis=1)
        assert np.array_equal(inside_got, inside_want), "the image circle's masks differ"
        assert 0 < int(inside_got.sum()) < w * h, "the frame must hold pixels inside and outside the circle"
        err = float(np.abs(fe[:, 4:7].astype(np.float64) - want[:, 4:7]).max())
        print(f"fisheye {w}x{h} fov {fov:.3f}: max component difference {err:.3g}")
        assert err <= 1e-6


# ---- 4. the lens ----------------------------------------------------------------------------------------
def test_the_lens_geometry():
    cfg = CFGS["40x36_of_a_ladder"]()
    _, ref = CAMERAS["lens"]
    R, focus = float(ref.lens_radius), float(ref.focus_distance)
    pos, _, _, right, up, _, fwd_n = [np.asarray(v, dtype=np.float64) for v in SR.frame_basis(CAM.uniform())]
    for s in SAMPLES:
        rec = SR.sample_rays(CAM.uniform(), cfg, ref, s).astype(np.float64)
        d = SR.sample_rays(CAM.uniform(), cfg, SR.Still(), s).astype(np.float64)[:, 4:7]          # the pinhole direction of the same sample
        off = rec[:, 0:3] - pos
        # 1e-6 relative to the numbers that are rounded: origin = position + off is one binary32 add per component, half an ulp of a coordinate of size |position| + R
        # (2^-24 relative, three components), on top of the five rounded operations behind off itself
        slack = 1e-6 * (float(np.linalg.norm(pos)) + R)
        assert float(np.linalg.norm(off, axis=1).max()) <= R + slack, "an origin lies outside the aperture"
        assert float(np.abs(off @ fwd_n).max()) <= slack, "an origin leaves the right / up plane"
        assert len(np.unique(_bits(rec[:, 0:3].astype(np.float32)), axis=0)) > rec.shape[0] // 2, "neighbouring pixels must not share a lens point"
        target = pos + d * focus
        reach = np.linalg.norm(d * focus - off, axis=1)
        back = rec[:, 0:3] + rec[:, 4:7] * reach[:, None]
        err = float(np.abs(back - target).max())
        assert err <= 1e-5 * focus, f"sample {s}: a ray misses its point of focus by {err:.3g}"
        assert float(np.abs(np.linalg.norm(rec[:, 4:7], axis=1) - 1).max()) <= 1e-6
    assert not np.array_equal(SR.sample_rays(CAM.uniform(), cfg, ref, 0)[:, 0:3], SR.sample_rays(CAM.uniform(), cfg, SR.Still(), 0)[:, 0:3]), "sample 0 is a lens sample"


def test_the_lens_points_cover_the_disk_evenly():
    N = 4096
    worst = 0.0
    for q in (0, 1, 40 * 17 + 5, 1919 * 1080):
        ru, rv = SR.lens_uv(q, np.arange(N))
        rr = np.sqrt(ru, dtype=np.float32)
        ang = rv * np.float32(6.28318548)
        x, y = rr * SR.sincos(ang, True), rr * SR.sincos(ang, False)
        shares = [float((((x >= 0) == a) & ((y >= 0) == b)).mean()) for a in (True, False) for b in (True, False)]
        inner = float((x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2 < 0.5).mean())
        print(f"pixel {q}: quadrant shares {['%.4f' % v for v in shares]}, inner half-area circle {inner:.4f}")
        worst = max([worst, abs(inner - 0.5)] + [abs(v - 0.25) for v in shares])
        assert all(abs(v - 0.25) <= 0.02 for v in shares) and abs(inner - 0.5) <= 0.02
    print(f"largest deviation {worst:.4f}")
    # ... and the records carry those points: pixel q of the frame at sample s
    cfg = CFGS["33x32_one_level"]()
    _, ref = CAMERAS["lens"]
    _, _, _, right, up, _, _ = SR.frame_basis(CAM.uniform())
    rec = SR.sample_rays(CAM.uniform(), cfg, ref, 7)
    ru, rv = SR.lens_uv(np.arange(33 * 32), 7)
    want_r = np.sqrt(ru.astype(np.float64)) * float(ref.lens_radius)
    off = rec[:, 0:3].astype(np.float64) - np.frombuffer(CAM.uniform(), np.float32)[0:3]
    assert np.allclose(np.linalg.norm(off, axis=1), want_r, rtol=1e-5, atol=1e-7)


# ---- 5. the surface -------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbols_exist_and_are_bound():
    L = B.lib()
    hdr, diag = _header("bhray.h"), _header("bhray_diag.h")
    for names, text, table in (({"bhray_accum_set_camera": 2, "bhray_still_camera_default": 1}, hdr, layouts.SYMBOLS), ({"bhray_still_sample_rays_host": 5}, diag, layouts.DIAG_SYMBOLS)):
        for name, nargs in names.items():
            assert re.search(r"\b(int|void)\s+%s\s*\(" % name, text), f"{name} is not declared"
            assert name in table and len(table[name][1]) == nargs, name
            assert len(getattr(L, name).argtypes) == nargs      # AttributeError: not exported
    assert not re.search(r"\bbhray_still_sample_rays_host\b", hdr), "the host form belongs to bhray_diag.h"
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "the addition is purely additive: the version stays"
    assert re.search(r"BHRAY_F_ALL\s*=\s*0xbfu", hdr), "no config flag was added"
    assert re.search(r"BHRAY_STILL_PINHOLE = 0, BHRAY_STILL_EQUIRECT = 1, BHRAY_STILL_FISHEYE = 2", hdr)
    assert (layouts.STILL_PINHOLE, layouts.STILL_EQUIRECT, layouts.STILL_FISHEYE) == (0, 1, 2) == (cameras.STILL_PINHOLE, cameras.STILL_EQUIRECT, cameras.STILL_FISHEYE)


def test_the_struct_layout():
    S = layouts.BhrayStillCamera
    assert C.sizeof(S) == 20
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("struct_size", 0), ("projection", 4), ("fisheye_fov", 8), ("lens_radius", 12), ("focus_distance", 16)]
    body = re.search(r"typedef struct bhray_still_camera \{(.*?)\} bhray_still_camera;", _header("bhray.h"), flags=re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+([a-z_]+);", body) == [("uint32_t", "struct_size"), ("uint32_t", "projection"), ("float", "fisheye_fov"), ("float", "lens_radius"), ("float", "focus_distance")]
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "bhray_layout.cpp")).read()
    assert "SZ(bhray_still_camera, 20)" in src and "OFF(bhray_still_camera, focus_distance, 16)" in src
    s = StillCamera.pinhole(lens_radius=0.25, focus_distance=9.0).struct()
    assert (s.struct_size, s.projection, s.lens_radius, s.focus_distance) == (20, 0, 0.25, 9.0)
    assert StillCamera.fisheye(2.0).struct().projection == 2 and StillCamera.equirect().struct().projection == 1


def test_refusals_that_need_no_device():
    L = B.lib()
    cfg = CFGS["33x32_one_level"]()
    out = np.zeros((33 * 32, 8), np.float32)
    p = out.ctypes.data_as(C.POINTER(layouts.BhrayRay))
    u = CAM.uniform()
    assert L.bhray_accum_set_camera(None, None) == E_INVALID
    L.bhray_still_camera_default(None)                            # no crash
    assert L.bhray_still_sample_rays_host(None, u, None, 0, p) == E_INVALID
    assert L.bhray_still_sample_rays_host(C.byref(cfg), None, None, 0, p) == E_INVALID
    assert L.bhray_still_sample_rays_host(C.byref(cfg), u, None, 0, None) == E_INVALID
    assert L.bhray_still_sample_rays_host(C.byref(cfg), u, None, 65536, p) == E_INVALID

    def bad(**kw):
        s = StillCamera().struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return L.bhray_still_sample_rays_host(C.byref(cfg), u, C.byref(s), 0, p)
    assert bad() == 0
    assert bad(struct_size=16) == E_INVALID and bad(struct_size=24) == E_INVALID
    assert bad(projection=3) == E_INVALID
    for fov in (0.0, -1.0, 6.3, float("nan"), float("inf")):
        assert bad(projection=2, fisheye_fov=fov) == E_INVALID, fov
    assert bad(projection=2, fisheye_fov=6.28318548) == 0 and bad(projection=0, fisheye_fov=float("nan")) == 0, "the fov is read for the fisheye only"
    for r in (-0.5, float("nan"), float("inf")):
        assert bad(lens_radius=r) == E_INVALID, r
    assert bad(projection=1, lens_radius=0.1, focus_distance=5.0) == E_INVALID and bad(projection=2, lens_radius=0.1, focus_distance=5.0) == E_INVALID
    for f in (0.0, -2.0, float("nan"), float("inf")):
        assert bad(lens_radius=0.1, focus_distance=f) == E_INVALID, f
    assert bad(lens_radius=0.0, focus_distance=float("nan")) == 0, "the focus is read with a lens only"


def test_the_hosts_carry_the_feature():
    assert hasattr(B.RayPass, "accum_set_camera") and B.StillCamera is StillCamera
    assert inspect.signature(B.Renderer.render_still).parameters["camera"].default is None
    assert inspect.signature(B.Renderer.save_still).parameters["camera"].default is None
    assert list(inspect.signature(cameras.still_rays).parameters) == ["camera", "cfg", "still_camera", "s"]
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert re.search(r"std::vector<float> render_still\(uint32_t samples, const bhray_still_camera\* still_camera = nullptr\)", hpp) and "bhray_accum_set_camera(" in hpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_stillcam.hip" in mk and "bhray_stillcam.o" in mk and "bhray_stillcam.h" in mk
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 21\. ", design, flags=re.M) and "bhray_accum_set_camera" in design
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn bhray_accum_set_camera(" in md and "pub struct bhray_still_camera" in md
    assert "bhray_accum_set_camera" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "still_camera_cost.py"))


def test_the_programs_arguments(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    src = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert "--still-camera" in src and "--lens" in src
    out = str(tmp_path / "o.f32")
    small = ["--base", "24", "14", "--levels", "1"]
    for bad_args in (["--spp", "4", "--still-camera"], ["--spp", "4", "--still-camera", "cube"], ["--spp", "4", "--still-camera", "fisheye"],
                     ["--spp", "4", "--still-camera", "fisheye", "0"], ["--spp", "4", "--still-camera", "fisheye", "7"], ["--spp", "4", "--still-camera", "fisheye", "nan"],
                     ["--still-camera", "equirect"], ["--lens", "0.1", "5"], ["--spp", "4", "--lens", "0.1"], ["--spp", "4", "--lens", "0", "5"],
                     ["--spp", "4", "--lens", "0.1", "0"], ["--spp", "4", "--lens", "-1", "5"], ["--spp", "4", "--still-camera", "equirect", "--lens", "0.1", "5"],
                     ["--spp-adaptive", "2", "6", "0.05", "--spp-round", "2", "--still-camera", "fisheye", "3", "--lens", "0.1", "5"],
                     ["--spp", "4", "--still-camera", "equirect", "--panorama", "8", "4"]):
        bad = subprocess.run([exe, out] + small + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and bad.stderr.strip() and not os.path.exists(out), bad_args
    if B.lib().bhray_device_count() > 0:
        return                                                     # with a device: tests/test_gpu_still_camera.py runs the program
    for good in (["--spp", "4", "--still-camera", "equirect"], ["--spp", "4", "--still-camera", "fisheye", "3.4"], ["--spp", "4", "--still-camera", "pinhole", "--lens", "0.1", "5"],
                 ["--spp-adaptive", "2", "6", "0.05", "--spp-round", "2", "--lens", "0.1", "5"]):
        r = subprocess.run([exe, out] + small + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (good, r.returncode, r.stderr)   # parsed and accepted: it fails at the device, not at the arguments
