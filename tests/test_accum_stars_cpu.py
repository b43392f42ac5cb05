"""CPU: point stars in stills (bhray_accum_set_stars) without a device.

  1. bhray_accum_stars_resolve_host - bhray_stars_resolve_host with the wrap of a whole equirect still - equals the restatement (tests/accum_stars_ref.py) in every
     word and count over np_ray's sample images 0 .. 2 of the default scene: wrap off for the pinhole's, wrap on (and off) for the equirect camera's; with
     wrap_x = 0 it is bhray_stars_resolve_host exactly.
  2. On a wrapped frame built from stars_ref.tie_frame a star on the seam edge belongs to exactly one pixel.
  3. Flux per sample is conserved.
  4. The coverage floors tests/test_gpu_accum_stars.py asks of the device's sample images, on np_ray's.
  5. The symbols, their bindings and the documents."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras, layouts
from bhusie_amd.cameras import StillCamera
from oracle import np_ray as N
from tests import accum_ref as A
from tests import accum_stars_ref as AS
from tests import common as T
from tests import stars_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
W, H = 40, 36
CAMERAS = {"pinhole": None, "equirect": StillCamera.equirect(), "fisheye": StillCamera.fisheye(3.14159274)}


def _cfg():
    """§18's 40 x 36 window of a two-level ladder: the whole width of its 40 x 37 last level from column 0, so an equirect still of it is periodic in x"""
    return B.ladder_for_frame((W, H), 3, 2)


@functools.lru_cache(maxsize=None)
def sample_image(camera, s, method=1):
    """np_ray's trace results for the rays of sample s under the named still camera: (36, 40, 4); a record without a direction (outside the fisheye's circle) is
    answered (0, 0, 0, -1) as the device answers it"""
    cam, bh = S.scene("default")
    rec = cameras.still_rays(cam, _cfg(), CAMERAS[camera], s)
    sc = N.Scene(*T.uniforms(camera=cam, black_hole=bh, integration_method=method), *T.textures())
    usable = (rec[:, 4:7] != 0.0).any(axis=1)
    out = np.zeros((rec.shape[0], 4), np.float32)
    out[:, 3] = -1.0
    out[usable] = N.trace_rays(sc, np.ascontiguousarray(rec[usable, 0:3]), np.ascontiguousarray(rec[usable, 4:7]))
    return out.reshape(H, W, 4)


@functools.lru_cache(maxsize=None)
def star_sum(camera, s, wrap, gain=1.0):
    return AS.star_sum(sample_image(camera, s), S.catalogue(), dict(gain=gain), wrap)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the host form -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_the_host_form_without_wrap_is_the_restatement_and_the_frame_form(s):
    f = sample_image("pinhole", s)
    want, st = star_sum("pinhole", s, False)
    got = B.accum_stars_resolve_host(f, S.catalogue())
    assert np.array_equal(_u32(got), _u32(want))
    assert np.array_equal(got[..., 3].astype(np.int64), st["accepted"])
    assert np.array_equal(_u32(got), _u32(B.stars_resolve_host(f, S.catalogue()))), "wrap_x = 0 is bhray_stars_resolve_host"
    p = layouts.BhrayStarParams.default(gain=3.5, min_area=2e-3)
    assert np.array_equal(_u32(B.accum_stars_resolve_host(f, S.catalogue(), p)), _u32(B.stars_resolve_host(f, S.catalogue(), p)))


@pytest.mark.parametrize("s", [0, 1])
def test_the_host_form_with_wrap_is_the_restatement_over_the_equirect_samples(s):
    f = sample_image("equirect", s)
    for wrap in (False, True):
        want, st = star_sum("equirect", s, wrap)
        got = B.accum_stars_resolve_host(f, S.catalogue(), wrap_x=wrap)
        assert np.array_equal(_u32(got), _u32(want)), wrap
        assert np.array_equal(got[..., 3].astype(np.int64), st["accepted"])
    off, on = star_sum("equirect", s, False)[0], star_sum("equirect", s, True)[0]
    assert not (off[:, [0, W - 1], 3] > 0).any(), "without the wrap the first and last columns are borders"
    assert np.array_equal(_u32(off[:, 1:W - 1]), _u32(on[:, 1:W - 1])), "the wrap changes the first and last columns only"
    assert not (on[[0, H - 1], :, 3] > 0).any(), "the top and bottom rows stay borders"


def test_null_and_invalid_arguments():
    L = B.lib()
    f = S.tie_frame()
    good = S.tie_stars([(3, 3), (4.5, 2)])
    out = np.full(f.shape, 7.0, np.float32)

    def call(frame=f, w=S.TIE_W, h=S.TIE_H, wrap=0, stars=good, n=2, params=None, dst=out):
        return L.bhray_accum_stars_resolve_host(frame.ctypes.data if frame is not None else None, w, h, wrap, stars.ctypes.data if stars is not None else None, n,
                                                C.byref(params) if params is not None else None, dst.ctypes.data if dst is not None else None)
    assert call() == 0 and out[..., 3].sum() == 2
    out[:] = 7.0
    assert call(frame=None) == E_INVALID and call(stars=None) == E_INVALID and call(dst=None) == E_INVALID and call(n=0) == E_INVALID
    assert call(w=0) == E_INVALID and call(h=0) == E_INVALID and call(w=40000) == E_INVALID
    bad = good.copy(); bad[1, 0] = np.nan
    assert call(stars=bad) == E_INVALID
    assert call(params=layouts.BhrayStarParams.default(max_footprint=0.3)) == E_INVALID and call(params=layouts.BhrayStarParams.default(struct_size=12)) == E_INVALID
    assert (out == 7.0).all()                                                    # a refused call writes nothing
    assert L.bhray_accum_set_stars(None, 1) == E_INVALID                         # no ctx


# ---- 2. the seam ----------------------------------------------------------------------------------------------------------------------------------------------------
ROLL = 4


def _rolled():
    """tie_frame with its columns rotated left by ROLL: frame column x holds tie column (x + ROLL) % TIE_W, so the seam between the last and the first column is the
    edge between tie columns ROLL - 1 and ROLL (x = ROLL - 0.5 in the frame plane), and the jump from tie column TIE_W - 1 back to 0 lies inside the frame - its
    footprints are 4 pixels wide and max_footprint = 0.05 (a pixel's diagonal is 0.022, theirs 0.0625 and more) turns them away"""
    return np.ascontiguousarray(np.roll(S.tie_frame(), -ROLL, axis=1))


def test_a_star_on_the_seam_edge_belongs_to_exactly_one_pixel():
    f = _rolled()
    seam = ROLL - 0.5
    pts = [(seam, 2.0), (seam, 2.5), (seam, 3.0), (seam, 4.5), (seam - 0.5, 3.0), (seam + 0.5, 2.0), (seam - 0.25, 1.5), (seam + 0.25, 4.0)]
    stars = S.tie_stars(pts)
    kw = dict(max_footprint=0.05)
    p = layouts.BhrayStarParams.default(**kw)
    want, st = AS.star_sum(f, stars, kw, True)
    got = B.accum_stars_resolve_host(f, stars, p, wrap_x=True)
    assert np.array_equal(_u32(got), _u32(want))
    owners = {}
    for y, x, k, rev in st["hits"]:
        assert not rev
        owners.setdefault(k, []).append((x, y))
    for k, (sx, sy) in enumerate(pts):
        tx, ty = S.tie_owner(sx, sy)                                             # the owner in tie_frame's columns
        assert owners.get(k) == [((tx - ROLL) % S.TIE_W, ty)], (k, sx, sy, owners.get(k))
    assert {o[0][0] for o in owners.values()} == {0, S.TIE_W - 1}, "the stars light the first and the last column"
    assert int(got[..., 3].sum()) == len(pts)
    plain = B.accum_stars_resolve_host(f, stars, p, wrap_x=False)
    assert not plain[..., 3].any(), "without the wrap both columns are borders and every one of these stars is lost"


# ---- 3. flux ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera,s,wrap", [("pinhole", 0, False), ("pinhole", 1, False), ("pinhole", 2, False), ("equirect", 0, True)])
def test_flux_per_sample_is_conserved(camera, s, wrap):
    """Sum over the lit pixels of add * max(A, min_area) against the summed flux * gain of the accepted stars (the restatement's hits).  Per pixel with n accepted
    stars: 1 / max(A, min_area), n products flux * inv, n additions into acc and the product with the gain - 2^-24 relative each, the additions relative to a
    partial sum that is at most the pixel's total because every term is >= 0: (3 + n) * 2^-24 of the pixel's total t.  The image's total is then off by at most
    sum((3 + n) t) / sum(t) * 2^-24, the t-weighted mean of 3 + n, which stays under §23's 4 * 2^-23 relative per channel while the weighted mean of n is at most 5:
    the test asserts that of its images from the restatement (a panorama's pixels near the poles hold up to 7 stars, its weighted mean is below 3).  Derived, not
    measured."""
    gain = 3.5
    f = sample_image(camera, s)
    want, st = star_sum(camera, s, wrap, gain)
    got = B.accum_stars_resolve_host(f, S.catalogue(), layouts.BhrayStarParams.default(gain=gain), wrap_x=wrap)
    assert np.array_equal(_u32(got), _u32(want))
    t = want[..., 0:3].astype(np.float64) * np.maximum(st["area"].astype(np.float64), float(np.float32(1e-7)))[..., None]
    weighted_n = (t * st["accepted"][..., None]).sum(axis=(0, 1)) / t.sum(axis=(0, 1))
    print(camera, s, "stars per pixel at most", int(st["accepted"].max()), "weighted mean", weighted_n)
    assert (weighted_n <= 5.0).all()
    area = np.maximum(st["area"].astype(np.float64), float(np.float32(1e-7)))
    lit = got[..., 3] > 0
    total = (got[..., 0:3].astype(np.float64) * area[..., None])[lit].sum(axis=0)
    cat = S.catalogue()
    flux = np.zeros(3, np.float64)
    for _, _, k, _ in st["hits"]:
        flux += cat[k, 3:6].astype(np.float64) * gain
    assert len(st["hits"]) == int(got[..., 3].sum()) >= 40
    rel = np.abs(total - flux) / flux
    print(camera, s, rel)
    assert (rel <= 4 * 2.0 ** -23).all(), rel


# ---- 4. the floors ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_floors_of_the_pinhole_samples():
    lit = []
    for s in range(5):
        fl = S.floors(star_sum("pinhole", s, False)[1])
        print(s, fl)
        assert fl["lit"] >= 40 and fl["reversed"] >= 10, (s, fl)
        lit.append(star_sum("pinhole", s, False)[0][..., 3] > 0)
    assert int((lit[0] != lit[1]).sum()) >= 20, "the lit sets of samples 0 and 1"
    tex = T.textures()[2]
    plain = A.mean(A.accumulate([sample_image("pinhole", s).reshape(-1, 4) for s in range(5)], tex))
    stars = AS.mean([AS.starred(sample_image("pinhole", s), S.catalogue(), None, tex)[0] for s in range(5)], tex)[0]
    assert int((_u32(plain) != _u32(stars)).any(axis=1).sum()) >= 100, "pixels of the mean that differ from the starless mean"


def test_the_floors_of_the_equirect_and_fisheye_samples_and_of_the_saturating_gain():
    add, st = star_sum("equirect", 0, True)
    assert int((add[:, [0, W - 1], 3] > 0).sum()) >= 5, "lit pixels in the first and last columns"
    assert S.floors(st)["footprints"] >= 1000
    f = sample_image("fisheye", 0)
    fadd, fst = star_sum("fisheye", 0, False)
    outside = f[..., 3] == -1.0
    assert int((fadd[..., 3] > 0).sum()) >= 300 and int(outside.sum()) >= 400 and not (fadd[outside, 3] > 0).any()
    tex = T.textures()[2]
    t = AS.starred(sample_image("pinhole", 0), S.catalogue(), dict(gain=1e6), tex)[0]
    assert int((t[..., 0:3] == 65504.0).any(axis=-1).sum()) >= 4 and float(t[np.isfinite(t)].max()) == 65504.0


# ---- 5. symbols, bindings, documents ----------------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_their_bindings():
    L = B.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bhray.h")).read(), flags=re.S)
    for name, nargs in {"bhray_accum_set_stars": 2, "bhray_accum_stars_resolve_host": 8}.items():
        assert hasattr(L, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == nargs == len(layouts.SYMBOLS[name][1]), name
        assert layouts.SYMBOLS[name][0] is C.c_int
    assert layouts.SYMBOLS["bhray_accum_set_stars"][1][1] is C.c_int32 and layouts.SYMBOLS["bhray_accum_stars_resolve_host"][1][3] is C.c_int32
    assert re.search(r"#define\s+BHRAY_VERSION_MINOR\s+5\b", text)


def test_the_hosts_and_the_documents_carry_the_feature():
    assert inspect.signature(B.RayPass.accum_set_stars).parameters["on"].default is False
    for fn in (B.Renderer.render_still, B.Renderer.save_still):
        assert inspect.signature(fn).parameters["stars"].default is False
    assert "wrap_x" in inspect.signature(B.accum_stars_resolve_host).parameters

    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    hpp = read("bhusie_amd", "csrc", "host", "renderer.hpp")
    assert "void set_still_stars(bool on)" in hpp and "bhray_accum_set_stars(" in hpp
    assert "dev_accum_set_stars(p.dev, on)" in read("bhusie_amd", "csrc", "bhray_group.hip"), "a multi-device ctx forwards the call as it does the filter"
    md = read("INTEGRATION.md")
    assert "pub fn bhray_accum_set_stars(" in md and "pub fn bhray_accum_stars_resolve_host(" in md
    assert "bhray_accum_set_stars" in read("README.md")
    design = read("DESIGN.md")
    assert re.search(r"^## 24\. ", design, flags=re.M) and "accum_star_kernel" in design and "bhray_accum_set_stars" in design


def test_the_programs_arguments(tmp_path):
    """bhray_render refuses --stars-seeded without --spp, with --spp-adaptive and with --lens before any device is touched"""
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "o.f32"
    for args in (["--stars-seeded", "100", "1"], ["--spp-adaptive", "2", "6", "0.1", "--stars-seeded", "100", "1"], ["--spp", "4", "--lens", "0.1", "10", "--stars-seeded", "100", "1"],
                 ["--spp", "4", "--stars-seeded", "0", "1"], ["--spp", "4", "--stars-seeded", "100"]):
        r = subprocess.run([exe, str(out), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--stars-seeded" in r.stderr and not out.exists(), (args, r.stderr)
