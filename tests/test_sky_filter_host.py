"""CPU: the sky filter's entry points (bhray_set_sky_filter, bhray_sky_pyramid_sizes, bhray_read_sky_pyramid_level) exist in the headers, the
library and every binding; bhray_sky_pyramid_sizes against the NumPy restatement (tests/sky_filter_ref.py); the refusals that need no device; the hosts carry the
feature."""
import ctypes as C
import inspect
import os
import re

import pytest

import bhusie_amd as B
from bhusie_amd import layouts
from tests import sky_filter_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PRODUCT = {"bhray_set_sky_filter": 2, "bhray_sky_pyramid_sizes": 5}
DIAG = {"bhray_read_sky_pyramid_level": 4}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


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


@pytest.mark.parametrize("w,h", [(5, 3), (1, 7), (512, 256), (37, 19), (4096, 2048), (1, 1), (32768, 1), (3, 32768), (2 ** 31, 1), (1, 2 ** 31 - 1)])
def test_pyramid_sizes_are_the_restatements(w, h):
    assert B.sky_pyramid_sizes(w, h) == S.sizes(w, h)
    got = B.sky_pyramid_sizes(w, h)
    assert got[0] == (w, h) and got[-1] == (1, 1) and len(got) <= 32
    for (a, b), (c, d) in zip(got, got[1:]):
        assert c == (a + 1) >> 1 and d == (b + 1) >> 1


def test_null_and_invalid_arguments_are_codes():
    L = B.lib()
    n, lw, lh = C.c_uint32(9), (C.c_uint32 * 32)(), (C.c_uint32 * 32)()
    assert L.bhray_sky_pyramid_sizes(0, 4, C.byref(n), lw, lh) == E_INVALID
    assert L.bhray_sky_pyramid_sizes(4, 0, C.byref(n), lw, lh) == E_INVALID
    assert L.bhray_sky_pyramid_sizes(2 ** 31 + 1, 4, C.byref(n), lw, lh) == E_INVALID      # a 33rd level would not fit lw[32]
    assert L.bhray_sky_pyramid_sizes(4, 2 ** 32 - 1, C.byref(n), lw, lh) == E_INVALID
    assert L.bhray_sky_pyramid_sizes(4, 4, None, lw, lh) == E_INVALID
    assert L.bhray_sky_pyramid_sizes(4, 4, C.byref(n), None, lh) == E_INVALID
    assert L.bhray_sky_pyramid_sizes(4, 4, C.byref(n), lw, None) == E_INVALID
    assert n.value == 9, "a refused call writes nothing"
    assert L.bhray_sky_pyramid_sizes(4, 4, C.byref(n), lw, lh) == 0 and n.value == 3
    buf = (C.c_uint16 * 16)()
    for mode in (0, 1, 2, -1):
        assert L.bhray_set_sky_filter(None, mode) == E_INVALID
    assert L.bhray_read_sky_pyramid_level(None, 1, buf, 4) == E_INVALID


def test_the_hosts_carry_the_feature():
    assert "mode" in inspect.signature(B.RayPass.set_sky_filter).parameters
    assert list(inspect.signature(B.RayPass.read_sky_pyramid_level).parameters)[1:] == ["level", "size"]
    src = inspect.getsource(B.Renderer)
    assert "self.sky_filter = False" in src and "set_sky_filter" in inspect.getsource(B.Renderer.save_image)
    hpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "renderer.hpp")).read()
    assert "bhray_set_sky_filter(ctx_" in hpp
    cpp = open(os.path.join(ROOT, "bhusie_amd", "csrc", "host", "bhray_render.cpp")).read()
    assert '"--sky-filter"' in cpp
    mk = open(os.path.join(ROOT, "bhusie_amd", "csrc", "Makefile")).read()
    assert "bhray_skyfilter.hip" in mk and "bhray_skyfilter.o" in mk
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn bhray_set_sky_filter(" in md and "pub fn bhray_sky_pyramid_sizes(" in md
