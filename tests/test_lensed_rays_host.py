"""CPU: the host side of lensed ray batches (bhray_set_mesh_lensing's BHRAY_LENS_RAYS) - the two constants in the header, the Python layouts and the Rust
text, the version unchanged and no symbol added; the rewritten comments; the kernel variant's rule in bhray_internal.h; the hosts' attribute; the C++ program's argument
rule, which needs no device."""
import os
import re
import subprocess

import bhusie_amd as B
from bhusie_amd import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_constants_agree_and_the_abi_is_the_same():
    hdr = _read("include", "bhray.h")
    m1 = re.search(r"#define BHRAY_LENS_FRAMES\s+(\d+)\b", hdr)
    m2 = re.search(r"#define BHRAY_LENS_RAYS\s+(\d+)\b", hdr)
    assert m1 and m2, "BHRAY_LENS_FRAMES / BHRAY_LENS_RAYS are not in include/bhray.h"
    assert (int(m1.group(1)), int(m2.group(1))) == (1, 2) == (layouts.LENS_FRAMES, layouts.LENS_RAYS) == (B.LENS_FRAMES, B.LENS_RAYS)
    assert re.search(r"#define BHRAY_VERSION_MINOR 5\b", hdr), "no symbol is added: the version stays"
    assert re.search(r"int bhray_set_mesh_lensing\(bhray_ctx\* ctx, int32_t on\);", hdr), "the signature is unchanged"
    assert len(layouts.SYMBOLS["bhray_set_mesh_lensing"][1]) == 2
    doc = _read("INTEGRATION.md")
    assert re.search(r"pub const BHRAY_LENS_FRAMES: i32 = 1;", doc) and re.search(r"pub const BHRAY_LENS_RAYS: i32 = 2;", doc)
    assert re.search(r"pub fn bhray_set_mesh_lensing\(ctx: \*mut bhray_ctx, on: i32\) -> c_int;", doc)


def test_the_comments_were_rewritten():
    hdr = _read("include", "bhray.h")
    assert "Not built: records under mesh lensing" not in hdr
    records = hdr[hdr.index("/* Ray records"):hdr.index("enum { BHRAY_HIT_NONE")]
    assert not re.search(r"not built", records, re.I), "the records' comment still says `not built`"
    assert "BHRAY_LENS_RAYS" in records and "first time crs.hit is true" in records
    paths = hdr[hdr.index("/* Ray paths"):hdr.index("typedef struct bhray_path_point")]
    assert re.search(r"Not built: paths under mesh lensing", paths), "paths under lensing stay not built, and the header says so"
    lensing = hdr[hdr.index("/* Lensed meshes"):hdr.index("int bhray_set_mesh_lensing")]
    for word in ("BHRAY_LENS_RAYS", "bhray_trace_rays_records", "bhray_accum_add", "bhray_trace_rays_paths"):
        assert word in lensing, word
    accum = hdr[hdr.index("/* Supersampled stills"):hdr.index("#define BHRAY_ACCUM_MAX_SAMPLES")]
    assert "without BHRAY_LENS_RAYS" in accum


def test_trace_resolve_keeps_lensed_ray_lists_and_folds_paths():
    src = _read("bhusie_amd", "csrc", "bhray_internal.h")
    # a lensed ray list and a lensed records request stay lensed; a path request folds to flat-space models
    assert "static_assert(trace_resolve({0, 2, false, true,  0, false, true}) == TraceVariant{0, 2, false, false, 0, false, true}" in src
    assert "static_assert(trace_resolve({1, 2, true,  true,  0, true,  false, true}) == TraceVariant{1, 2, false, false, 0, false, true, true}" in src
    assert "static_assert(trace_resolve({0, 2, false, false, 0, false, true, true, true}) == TraceVariant{0, 1, false, false, 0, false, true, true, true}" in src
    assert "static_assert(trace_resolve({1, 2, true,  true,  0, true,  false, false, true}) == TraceVariant{1, 1, false, false, 0, false, true, true, true}" in src
    assert "TraceVariant{0, 1, false, false, 0, false, true}, \"trace_resolve\");   // ... and flat-space models" not in src, "the old fold is still pinned"
    ker = _read("bhusie_amd", "csrc", "bhray_kernels.hip")
    assert "static_assert(!(LENSED && PATHS)" in ker
    assert not re.search(r"static_assert\(!RAYS \|\| \([^)]*!LENSED", ker), "LENSED && RAYS is still forbidden"
    assert "+ 4 + 4 + 4 + 4," in ker, "TRACE_BUILDS.n grows by the four lensed ray-list / record kernels"
    api = _read("bhusie_amd", "csrc", "bhray_api.hip")
    assert re.search(r"int rays_refused\(bhray_dev\* c, const char\* name, bool path_call", api)
    assert "ray batches under mesh lensing are not built" in api, "the refusal keeps its message"


def test_the_hosts_have_the_attribute():
    r = B.Renderer.__new__(B.Renderer)                            # no ctx: the rule is plain arithmetic on two attributes
    r.mesh_lensing, r.lens_ray_batches = False, True
    assert r._lensing_word() == 0
    r.mesh_lensing = True
    assert r._lensing_word() == (B.LENS_FRAMES | B.LENS_RAYS) == 3
    r.lens_ray_batches = False
    assert r._lensing_word() == B.LENS_FRAMES == 1
    hpp = _read("bhusie_amd", "csrc", "host", "renderer.hpp")
    assert re.search(r"bool lens_ray_batches = false;", hpp) and "BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS" in hpp
    assert re.search(r"int32_t lensing_applied_ = 0;", hpp), "the C++ host compares the word it last sent, not its truth"
    cpp = _read("bhusie_amd", "csrc", "host", "bhray_render.cpp")
    assert "lens_ray_batches" in cpp


def test_the_program_refuses_a_path_under_lensed_mesh_without_a_device(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "o.f32"
    r = subprocess.run([exe, str(out), "--lensed-mesh", "--path", "3", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--lensed-mesh" in r.stderr and not out.exists()
