"""CPU: the host side of point stars (bhray_set_stars) - the symbols and their declarations in the two headers, the struct layouts in every binding,
NULL and invalid arguments of the calls that need no device, and bhray_render's --stars-seeded argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from tests import stars_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PRODUCT = {"bhray_star_params_default": 1, "bhray_set_stars": 4, "bhray_star_grid_size": 2, "bhray_star_cell": 3, "bhray_stars_resolve_host": 7}
DIAG = {"bhray_diag_star_image": 6, "bhray_diag_stars_pixel_info_host": 7}


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_symbols_and_declarations():
    L = B.lib()
    for names, text, table in ((PRODUCT, _read("include", "bhray.h"), layouts.SYMBOLS), (DIAG, _read("include", "bhray_diag.h"), layouts.DIAG_SYMBOLS)):
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for name, nargs in names.items():
            assert hasattr(L, name), name
            m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
            assert m, f"{name} is not declared"
            assert m.group(1).count(",") + 1 == nargs == len(table[name][1]), name
    hdr = _read("include", "bhray.h")
    assert re.search(r"#define\s+BHRAY_MAX_STARS\s+\(1u << 22\)", hdr) and re.search(r"#define\s+BHRAY_STARS_MAX_CELLS\s+64u", hdr)
    assert re.search(r"#define\s+BHRAY_VERSION_MINOR\s+5\b", hdr)
    assert layouts.MAX_STARS == 1 << 22 and layouts.STARS_MAX_CELLS == S.MAX_CELLS == 64


def test_struct_layouts_in_every_binding():
    assert C.sizeof(layouts.BhrayStar) == 24 and layouts.BhrayStar.dir.offset == 0 and layouts.BhrayStar.flux.offset == 12
    P = layouts.BhrayStarParams
    assert C.sizeof(P) == 16 and (P.struct_size.offset, P.gain.offset, P.min_area.offset, P.max_footprint.offset) == (0, 4, 8, 12)
    assert B.STAR_PIXEL_INFO_DTYPE.itemsize == 32 and B.STAR_PIXEL_INFO_DTYPE.fields["area"][1] == 24
    lay = _read("bhusie_amd", "csrc", "bhray_layout.cpp")
    assert "SZ(bhray_star, 24);" in lay and "SZ(bhray_star_params, 16);" in lay and "OFF(bhray_star, flux, 12)" in lay and "OFF(bhray_star_params, max_footprint, 12)" in lay
    doc = _read("INTEGRATION.md")
    for decl in ("pub struct bhray_star", "pub struct bhray_star_params", "pub fn bhray_set_stars", "pub fn bhray_stars_resolve_host", "pub fn bhray_star_cell", "pub fn bhray_star_grid_size"):
        assert decl in doc, decl
    hpp = _read("bhusie_amd", "csrc", "host", "renderer.hpp")
    assert "void set_stars(" in hpp and "star_catalogue(" in hpp


def test_the_defaults():
    p = layouts.BhrayStarParams()
    B.lib().bhray_star_params_default(C.byref(p))
    d = layouts.BhrayStarParams.default()
    assert bytes(p) == bytes(d) and p.struct_size == 16 and p.gain == 1.0 and p.min_area == np.float32(1e-7) and p.max_footprint == 0.25
    B.lib().bhray_star_params_default(None)                                     # a NULL is ignored


def test_null_and_invalid_arguments():
    L = B.lib()
    f = S.tie_frame()
    good = S.tie_stars([(3, 3), (4.5, 2)])
    out = np.full(f.shape, 7.0, np.float32)

    def call(frame=f, w=S.TIE_W, h=S.TIE_H, stars=good, n=None, params=None, dst=out):
        return L.bhray_stars_resolve_host(frame.ctypes.data if frame is not None else None, w, h, stars.ctypes.data if stars is not None else None,
                                          len(stars) if n is None and stars is not None else (n or 0), C.byref(params) if params is not None else None,
                                          dst.ctypes.data if dst is not None else None)
    assert call() == 0 and (out[..., 3].sum() == 2)
    out[:] = 7.0
    assert call(frame=None) == E_INVALID and call(stars=None) == E_INVALID and call(dst=None) == E_INVALID and call(n=0) == E_INVALID
    assert call(w=0) == E_INVALID and call(h=0) == E_INVALID and call(w=40000) == E_INVALID
    for k, v in ((0, np.nan), (1, np.inf), (3, -1e-9), (4, np.nan), (5, np.inf)):
        bad = good.copy(); bad[1, k] = v
        assert call(stars=bad) == E_INVALID, (k, v)
    bad = good.copy(); bad[0, 0:3] = 0.0
    assert call(stars=bad) == E_INVALID
    D = layouts.BhrayStarParams.default
    for p in (D(gain=0.0), D(gain=-1.0), D(gain=np.inf), D(gain=np.nan), D(min_area=0.0), D(min_area=np.inf), D(min_area=np.nan), D(max_footprint=0.0),
              D(max_footprint=0.2500001), D(max_footprint=np.nan), D(struct_size=12)):
        assert call(params=p) == E_INVALID, bytes(p)
    assert (out == 7.0).all()                                                    # a refused call writes nothing
    assert call(params=D(max_footprint=0.25, gain=2.0)) == 0
    assert L.bhray_set_stars(None, good.ctypes.data, 2, None) == E_INVALID       # no ctx
    assert L.bhray_diag_star_image(None, f.ctypes.data, S.TIE_W, S.TIE_H, None, out.ctypes.data) == E_INVALID
    info = np.zeros(f.shape[:2], B.STAR_PIXEL_INFO_DTYPE)
    assert L.bhray_diag_stars_pixel_info_host(f.ctypes.data, S.TIE_W, S.TIE_H, good.ctypes.data, 2, None, None) == E_INVALID
    assert L.bhray_diag_stars_pixel_info_host(f.ctypes.data, S.TIE_W, S.TIE_H, good.ctypes.data, 2, None, info.ctypes.data) == 0 and int(info["accepted"].sum()) == 2


def test_star_array_takes_the_three_forms():
    s = assets.star_catalogue(5, 3)
    a, n = B.star_array(s)
    assert n == 5 and a.dtype == np.float32 and a.flags.c_contiguous
    arr = (layouts.BhrayStar * 5)()
    for i in range(5):
        arr[i].dir[:] = s[i, 0:3].tolist(); arr[i].flux[:] = s[i, 3:6].tolist()
    b, n = B.star_array(arr)
    assert n == 5 and np.array_equal(a, b)
    assert B.star_array(None)[1] == 0 and B.star_array(np.zeros((0, 6)))[1] == 0
    with pytest.raises(ValueError):
        B.star_array(np.zeros((4, 5)))


@pytest.mark.parametrize("args", [["--stars-seeded"], ["--stars-seeded", "10"], ["--stars-seeded", "0", "1"], ["--stars-seeded", "-3", "1"], ["--stars-seeded", "4194305", "1"],
                                  ["--stars-seeded", "ten", "1"], ["--stars-seeded", "10", "-1"], ["--stars-seeded", "10", "1x"]], ids=lambda a: " ".join(a[1:]) or "none")
def test_bhray_render_refuses_bad_stars_seeded_arguments_before_any_device_is_touched(args, tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    r = subprocess.run([exe, "--handoff", "sky", "1", str(tmp_path / "o.bin"), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--stars-seeded needs" in r.stderr and not (tmp_path / "o.bin").exists()
