"""CPU: the point-star pass (bhray_set_stars) without a device - the library's host arithmetic and bhray_stars_resolve_host, which runs the kernel's
per-pixel function on the host, held to tests/stars_ref.py, the NumPy restatement, in every word; the exact ties of rule 5 on a synthetic frame; flux conservation;
and the coverage floors tests/test_gpu_stars.py asks of the device's frames, on np_ray's frames of the same scenes."""
import functools

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from oracle import np_ray as N
from tests import common as T
from tests import stars_ref as S

SEED, scene, catalogue, check_floors = S.SEED, S.scene, S.catalogue, S.check_floors
W, H = 40, 36


@functools.lru_cache(maxsize=None)
def frame(name, method):
    cam, bh = scene(name)
    return N.render_level(N.Scene(*T.uniforms(camera=cam, black_hole=bh, integration_method=method), *T.textures()), (W, H))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------------------------------------------
def test_grid_size():
    for n, want in ((0, 1), (1, 1), (12, 1), (13, 2), (2000, 16), (1 << 22, 1024)):
        assert B.star_grid_size(n) == S.grid_size(n) == want
    assert B.star_grid_size(120000) == 128
    g = layouts.C.c_uint32(7)
    assert B.lib().bhray_star_grid_size((1 << 22) + 1, layouts.C.byref(g)) == -1 and g.value == 7
    assert B.lib().bhray_star_grid_size(5, None) == -1


def test_cells_of_seeded_directions_and_of_the_cubes_ties():
    rng = np.random.default_rng(11)
    d = rng.standard_normal((100000, 3)).astype(np.float32)
    d[::7] *= np.float32(1e-20); d[::11] *= np.float32(1e20)                     # need not be unit length
    for G in (1, 16, 1024):
        assert np.array_equal(B.star_cells(d[:: (1 if G == 16 else 10)], G), S.cells(d[:: (1 if G == 16 else 10)], G))
    ties = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float32)
    assert len(ties) == 26
    for G in (1, 2, 16):
        got = B.star_cells(ties, G)
        assert np.array_equal(got, S.cells(ties, G))
        face = got // (G * G)
        want = [0 if x > 0 else 1 if x < 0 else 2 if y > 0 else 3 if y < 0 else 4 if z > 0 else 5 for x, y, z in ties]       # ties go to x, then y
        assert face.tolist() == want
    c = layouts.C.c_uint32()
    L = B.lib()
    f3 = layouts.C.c_float * 3
    for bad in ((0.0, 0.0, 0.0), (np.nan, 1.0, 0.0), (np.inf, 0.0, 0.0)):
        assert L.bhray_star_cell(f3(*bad), 16, layouts.C.byref(c)) == -1
    for G in (0, 3, 2048):
        assert L.bhray_star_cell(f3(1.0, 0.0, 0.0), G, layouts.C.byref(c)) == -1


def test_the_sorted_order_is_cell_then_index():
    s = catalogue()
    G, order, prefix = S.build_index(s)
    assert G == 16 and prefix[-1] == 2000 and len(prefix) == 6 * 256 + 1
    c = S.cells(s[:, 0:3], G)
    keys = list(zip(c[order].tolist(), order.tolist()))
    assert keys == sorted(keys)
    assert all((c[order[prefix[k]:prefix[k + 1]]] == k).all() for k in range(6 * 256))


def test_the_seeded_catalogue():
    s = catalogue()
    assert s.shape == (2000, 6) and s.dtype == np.float32 and np.array_equal(s, assets.star_catalogue(2000, SEED))
    assert not np.array_equal(s, assets.star_catalogue(2000, SEED + 1))
    n = np.linalg.norm(s[:, 0:3].astype(np.float64), axis=1)
    assert np.abs(n - 1).max() < 1e-6 and (s[:, 3:6] > 0).all() and np.isfinite(s).all()
    assert np.abs(s[:, 0:3].mean(axis=0)).max() < 0.05                          # uniform on the sphere: the mean direction of 2000 is near 0 (sigma 0.013)
    assert np.array_equal(assets.star_catalogue(500, SEED), s[:500])              # star i does not depend on n


def test_stars_from_uv_inverts_the_sky_passes_map():
    rng = np.random.default_rng(3)
    u, v = rng.uniform(0.01, 0.99, 200), rng.uniform(0.01, 0.99, 200)
    d = assets.stars_from_uv(u, v).astype(np.float64)
    theta = np.arctan2(np.hypot(d[:, 0], d[:, 2]), d[:, 1])
    phi = np.arctan2(d[:, 2], d[:, 0])
    assert np.abs(np.mod((phi + 2.6 * np.pi) / (2 * np.pi), 1.0) - u).max() < 1e-5 and np.abs((np.pi - theta) / np.pi - v).max() < 1e-5


# ---- the restatement on np_ray's frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("name", ["default", "nodisk", "diag"])
def test_the_host_form_is_the_restatement_in_every_word(name, method):
    f = frame(name, method)
    want, st = S.resolve(f, catalogue())
    fl = S.floors(st)
    print(name, method, fl)
    assert np.array_equal(_u32(B.stars_resolve_host(f, catalogue())), _u32(want))
    info = B.stars_pixel_info_host(f, catalogue())
    for k in ("state", "faces", "cells", "tested", "accepted", "reversed"):
        assert np.array_equal(info[k], st[k]), k
    assert np.array_equal(_u32(info["area"]), _u32(st["area"]))
    check_floors(fl, name)


@pytest.mark.parametrize("kw", [dict(gain=3.5), dict(min_area=2e-3), dict(max_footprint=0.05), dict(gain=0.25, min_area=1e-3, max_footprint=0.1)], ids=str)
def test_the_parameters(kw):
    f = frame("nodisk", 1)
    want, st = S.resolve(f, catalogue(), **kw)
    got = B.stars_resolve_host(f, catalogue(), layouts.BhrayStarParams.default(**kw))
    assert np.array_equal(_u32(got), _u32(want))
    if "max_footprint" in kw:
        assert (st["state"] == 1).sum() > S.floors(S.resolve(f, catalogue())[1])["by_size"]


def test_the_crowded_cell():
    f = frame("default", 1)
    cat = S.crowded_catalogue(f[5, 5, 0:3])
    want, st = S.resolve(f, cat)
    fl = S.floors(st)
    print(fl)
    check_floors(fl, "crowded")
    assert np.array_equal(_u32(B.stars_resolve_host(f, cat)), _u32(want))


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirrored"])
def test_a_star_on_a_corner_an_edge_or_a_centre_lights_exactly_the_pixel_the_rule_names(mirror):
    f = S.tie_frame(mirror)
    pts = S.tie_points()
    stars = S.tie_stars(pts)
    want, st = S.resolve(f, stars)
    assert np.array_equal(_u32(B.stars_resolve_host(f, stars)), _u32(want))
    owners = {}
    for y, x, k, rev in st["hits"]:
        assert rev == mirror                                                     # the mirrored frame is accepted through the reversed-sign form
        owners.setdefault(k, []).append((x, y))
    for k, (sx, sy) in enumerate(pts):
        assert owners.get(k) == [S.tie_owner(sx, sy, mirror)], (k, sx, sy, owners.get(k))
    # every star's flux went to its pixel alone: A is 2^-12 exactly, so flux / A is exact
    inv = np.float32(4096.0)
    for k, (sx, sy) in enumerate(pts):
        x, y = S.tie_owner(sx, sy, mirror)
        assert st["accepted"][y, x] >= 1 and st["area"][y, x] == np.float32(2.0 ** -12)
    total = np.zeros(3, np.float64)
    for k in range(len(pts)):
        total += stars[k, 3:6].astype(np.float64) * float(inv)
    assert np.allclose(want[..., 0:3].astype(np.float64).sum(axis=(0, 1)), total, rtol=1e-6, atol=0)


@pytest.mark.parametrize("bad", ["nan", "inf", "colour"])
def test_a_pixel_that_is_no_finite_direction_takes_its_four_corners_with_it(bad):
    f = S.tie_frame()
    f[3, 4] = {"nan": (np.nan, 0.05, 1.0, 0.0), "inf": (0.06, np.inf, 1.0, 0.0), "colour": (0.0625, 0.046875, 1.0, 1.0)}[bad]
    stars = S.tie_stars([(x + 0.25, y + 0.25) for y in range(S.TIE_H) for x in range(S.TIE_W)])
    want, st = S.resolve(f, stars)
    assert np.array_equal(_u32(B.stars_resolve_host(f, stars)), _u32(want))
    has = st["state"] != 3
    expect = np.zeros((S.TIE_H, S.TIE_W), bool)
    expect[1:-1, 1:-1] = True
    expect[2:5, 3:6] = False                                                     # the pixel's four corners are those of the 3 x 3 block around it
    assert np.array_equal(has, expect)
    assert np.array_equal(st["accepted"] > 0, expect)                            # and every footprint that is left owns the star a quarter pixel off its centre


@pytest.mark.parametrize("w,h,footprints", [(1, 1, 0), (2, 2, 0), (3, 3, 1), (5, 3, 3)])
def test_tiny_frames(w, h, footprints):
    f = S.tie_frame(w=w, h=h)
    stars = S.tie_stars([(x, y) for y in range(h) for x in range(w)])
    want, st = S.resolve(f, stars)
    got = B.stars_resolve_host(f, stars)
    assert np.array_equal(_u32(got), _u32(want))
    assert int((st["state"] != 3).sum()) == footprints == int((got[..., 3] > 0).sum())


def test_flux_is_conserved():
    """Sum over pixels of add * max(A, min_area) against the summed flux of the stars inside the region that has footprints.  Per star: 1 / A, flux * inv and the
    addition into acc are three rounded operations, 2^-24 relative each; the order of the sum moves the total by no more than the additions' own rounding.  Bound:
    4 * 2^-23 relative per channel (derived, not measured; the stars lie on the quarter-pixel grid, where the inside test is exact)."""
    rng = np.random.default_rng(5)
    n = 120
    pts = np.stack([rng.integers(-4, 4 * S.TIE_W + 1, n) / 4.0, rng.integers(-4, 4 * S.TIE_H + 1, n) / 4.0], axis=1)
    flux = rng.uniform(1e-7, 1e-5, (n, 3)).astype(np.float32)
    stars = S.tie_stars(pts, flux)
    f = S.tie_frame()
    got = B.stars_resolve_host(f, stars)
    info = B.stars_pixel_info_host(f, stars)
    inside = (pts[:, 0] >= 0.5) & (pts[:, 0] < S.TIE_W - 1.5) & (pts[:, 1] >= 0.5) & (pts[:, 1] < S.TIE_H - 1.5)
    assert 40 <= inside.sum() <= n - 20 and int(got[..., 3].sum()) == int(inside.sum())
    area = np.maximum(info["area"].astype(np.float64), 1e-7)
    total = (got[..., 0:3].astype(np.float64) * area[..., None]).sum(axis=(0, 1))
    want = flux[inside].astype(np.float64).sum(axis=0)
    rel = np.abs(total - want) / want
    print(rel)
    assert (rel <= 4 * 2.0 ** -23).all(), rel
