"""-m gpu: point stars (bhray_set_stars) held to tests/stars_ref.py, the NumPy restatement, in every 16-bit word: the pass over the device's own
RGBA32F frame (read_hdr) and the device's own starless sky image - so nothing of the comparison depends on how the frame was traced or the sky sampled -, the
kernel over supplied frames (bhray_diag_star_image: exact ties, frames smaller than a tile, partial tiles), the catalogue's state, and what the pass must not touch."""
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from tests import common as T
from tests import post_ref as P
from tests import stars_ref as S

pytestmark = pytest.mark.gpu
SEED, scene, catalogue, check_floors = S.SEED, S.scene, S.catalogue, S.check_floors
E_INVALID, E_STATE = -1, -5


def _cfg(kind):
    """window: §18's 40 x 36 window of a two-level ladder; single: the 33 x 32 single-level frame"""
    return B.ladder_for_frame((40, 36), 3, 2) if kind == "window" else B.ladder_from_base((33, 32), 3, 1)


def _rp(kind="window", name="default", method=1, stars=None, **kw):
    cam, bh = scene(name)
    rp = B.RayPass(_cfg(kind), device=0, **kw)
    rp.set_textures(*T.textures())
    rp.set_uniforms(*T.uniforms(camera=cam, black_hole=bh, integration_method=method))
    if stars is not None:
        rp.set_stars(stars)
    return rp


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float16
    bad = (_bits(got) != _bits(want)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:5].tolist()}"


def _starred(rp, cat, what, **params):
    """resolve the last frame without and with the catalogue; hold the second image to the restatement over the first and the device's frame"""
    rp.set_stars(None)
    rp.resolve_sky()
    frame, plain = rp.read_hdr(), rp.read_sky()
    rp.set_stars(cat, layouts.BhrayStarParams.default(**params) if params else None)
    rp.resolve_sky()
    got = rp.read_sky()
    add, st = S.resolve(frame, cat, **params)
    _same(got, S.apply(plain, add), what)
    return frame, plain, got, st


# ---- 1. and 2.: the device's own frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("name", ["default", "nodisk"])
@pytest.mark.parametrize("kind", ["window", "single"])
def test_the_pass_is_the_restatement_in_every_word(kind, name, method):
    rp = _rp(kind, name, method)
    rp.render()
    for filt in (0, 1):
        rp.set_sky_filter(filt)
        _, plain, got, st = _starred(rp, catalogue(), f"{kind} {name} filter {filt}")
        fl = S.floors(st)
        print(kind, name, method, filt, fl)
        assert fl["lit"] >= 10 and int((_bits(got) != _bits(plain)).any(axis=-1).sum()) >= 10
        if kind == "window":
            check_floors(fl, name)
    rp.close()


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_floors_of_the_diagonal_camera_and_the_crowded_cell_on_the_devices_frames(method):
    rp = _rp("window", "diag", method)
    rp.render()
    _, _, _, st = _starred(rp, catalogue(), "diag")
    print(S.floors(st))
    check_floors(S.floors(st), "diag")
    rp.close()
    rp = _rp("window", "default", method)
    rp.render()
    frame = rp.read_hdr()
    _, _, _, st = _starred(rp, S.crowded_catalogue(frame[5, 5, 0:3]), "crowded")
    print(S.floors(st))
    check_floors(S.floors(st), "crowded")
    rp.close()


@pytest.mark.parametrize("params", [dict(gain=3.5), dict(min_area=2e-3, max_footprint=0.05)], ids=str)
def test_the_parameters(params):
    rp = _rp("window", "nodisk", 1)
    rp.render()
    _starred(rp, catalogue(), str(params), **params)
    rp.close()


# ---- 3.: the kernel over supplied frames --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    rp = _rp("single")
    yield rp
    rp.close()


def _image(rp, frame, stars, sky_in=None, **params):
    rp.set_stars(stars, layouts.BhrayStarParams.default(**params) if params else None)
    got = rp.star_image(frame, sky_in)
    add, st = S.resolve(frame, stars, **params)
    base = np.zeros(frame.shape, np.float16) if sky_in is None else sky_in
    _same(got, S.apply(base, add), "star_image")
    return got, add, st


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirrored"])
def test_exact_ties(ctx, mirror):
    pts = S.tie_points()
    stars = S.tie_stars(pts)
    got, add, st = _image(ctx, S.tie_frame(mirror), stars)
    owners = {}
    for y, x, k, rev in st["hits"]:
        assert rev == mirror
        owners.setdefault(k, []).append((x, y))
    assert owners == {k: [S.tie_owner(sx, sy, mirror)] for k, (sx, sy) in enumerate(pts)}
    assert int((got[..., 0] > 0).sum()) == len({v[0] for v in owners.values()}) and int(add[..., 3].sum()) == len(pts)


@pytest.mark.parametrize("bad", ["nan", "inf", "colour"])
def test_a_bad_pixel_takes_its_four_corners_with_it(ctx, bad):
    f = S.tie_frame()
    f[3, 4] = {"nan": (np.nan, 0.05, 1.0, 0.0), "inf": (0.06, np.inf, 1.0, 0.0), "colour": (0.0625, 0.046875, 1.0, 1.0)}[bad]
    stars = S.tie_stars([(x + 0.25, y + 0.25) for y in range(S.TIE_H) for x in range(S.TIE_W)])
    rng = np.random.default_rng(2)
    sky_in = rng.uniform(0, 2, f.shape).astype(np.float16)
    got, _, _ = _image(ctx, f, stars, sky_in)
    expect = np.zeros((S.TIE_H, S.TIE_W), bool)
    expect[1:-1, 1:-1] = True
    expect[2:5, 3:6] = False
    assert np.array_equal((_bits(got) != _bits(sky_in)).any(axis=-1), expect)
    assert np.array_equal(_bits(got[..., 3]), _bits(sky_in[..., 3]))              # alpha is kept


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (5, 3), (70, 19)])
def test_tiny_frames_and_partial_tiles(ctx, w, h):
    f = S.tie_frame(w=w, h=h)
    rng = np.random.default_rng(w * 100 + h)
    n = max(4, w * h // 2)
    pts = np.stack([rng.integers(-2, 4 * w + 2, n) / 4.0, rng.integers(-2, 4 * h + 2, n) / 4.0], axis=1)
    got, add, st = _image(ctx, f, S.tie_stars(pts, rng.uniform(1e-7, 1e-5, (n, 3)).astype(np.float32)))
    assert int((st["state"] != 3).sum()) == max(w - 2, 0) * max(h - 2, 0)
    if w >= 3 and h >= 3:
        assert (add[..., 3] > 0).any()
    else:
        assert not _bits(got).any()


def test_a_flux_that_overflows_binary16_stores_65504(ctx):
    f = S.tie_frame()
    stars = S.tie_stars([(3, 3), (4, 3), (5, 3)], flux=np.array([[1e3, 20.0, 1e-6], [3e35, 3e35, 3e35], [15.0, 16.0, 1e30]], np.float32))
    sky_in = np.zeros(f.shape, np.float16)
    sky_in[3, 5, 1] = 2.0; sky_in[3, 3, 2] = np.inf                               # an infinite sky word comes down to 65504 too
    got, add, _ = _image(ctx, f, stars, sky_in)
    assert np.isinf(add[3, 4, 0:3]).all()                                        # 3e35 * 4096 overflows binary32
    assert got[3, 3].tolist() == [65504.0, 65504.0, 65504.0, 0.0]
    assert got[3, 4].tolist() == [65504.0, 65504.0, 65504.0, 0.0]
    assert got[3, 5].tolist() == [61440.0, 65504.0, 65504.0, 0.0]                # 15 * 4096 fits; 2 + 16 * 4096 does not
    assert np.isfinite(got.astype(np.float32)).all()


# ---- 4.: the catalogue's state ------------------------------------------------------------------------------------------------------------------------------------
def test_removing_the_catalogue_gives_the_bits_of_a_ctx_that_never_saw_one():
    never = _rp("single")
    never.render(); never.resolve_display()
    want_sky, want_disp = never.read_sky(), never.read_display()
    never.close()
    rp = _rp("single", stars=catalogue())
    rp.render(); rp.resolve_display()
    assert not np.array_equal(_bits(rp.read_sky()), _bits(want_sky))
    rp.set_stars(None)
    rp.render(); rp.resolve_display()
    assert np.array_equal(_bits(rp.read_sky()), _bits(want_sky)) and np.array_equal(rp.read_display(), want_disp)
    with pytest.raises(B.BhrayError) as e:
        rp.star_image(S.tie_frame())
    assert e.value.code == E_STATE
    rp.set_stars(np.zeros((0, 6), np.float32))                                    # removing twice is fine
    rp.close()


def test_replacing_the_catalogue_with_four_frames_in_flight():
    rp = _rp("window", frames_in_flight=4)
    cats = [catalogue(), assets.star_catalogue(2000, SEED + 1)]
    pinned = [B.PinnedFrame(36, 40, channels16=True) for _ in range(8)]
    tickets, frames, which = [], [], []
    for i in range(8):
        rp.set_uniforms(*T.uniforms(integration_method=1, time=0.25 * i, camera=B.Camera(position=(0.2 * i, 0.0, -19.0))))
        rp.render()
        if i % 2 == 0:
            rp.set_stars(cats[(i // 2) % 2])                                     # between a render and its resolve, earlier frames still in flight
        rp.resolve_sky()
        tickets.append(rp.read_sky_async(pinned[i]))
        frames.append(rp.read_hdr()); which.append((i // 2) % 2)
    rp.set_stars(None)
    for i in range(8):
        rp.wait_read(tickets[i])
        rp.set_uniforms(*T.uniforms(integration_method=1, time=0.25 * i, camera=B.Camera(position=(0.2 * i, 0.0, -19.0))))
        rp.render(); rp.resolve_sky()
        plain = rp.read_sky()
        assert np.array_equal(rp.read_hdr().view(np.uint32), frames[i].view(np.uint32))
        _same(pinned[i].array, S.apply(plain, S.resolve(frames[i], cats[which[i]])[0]), f"frame {i}")
    for b in pinned:
        b.free()
    rp.close()


def test_a_refused_call_leaves_the_catalogue_in_force():
    rp = _rp("single", stars=catalogue())
    rp.render(); rp.resolve_sky()
    want = rp.read_sky()
    L = B.lib()
    bad = catalogue().copy(); bad[17, 1] = np.nan
    zero = catalogue().copy(); zero[3, 0:3] = 0.0
    neg = catalogue().copy(); neg[5, 4] = -1.0
    for s in (bad, zero, neg):
        assert L.bhray_set_stars(rp._h, s.ctypes.data, len(s), None) == E_INVALID
    assert L.bhray_set_stars(rp._h, bad.ctypes.data, (1 << 22) + 1, None) == E_INVALID
    for p in (layouts.BhrayStarParams.default(max_footprint=0.3), layouts.BhrayStarParams.default(min_area=0.0), layouts.BhrayStarParams.default(struct_size=8)):
        assert L.bhray_set_stars(rp._h, catalogue().ctypes.data, 2000, layouts.C.byref(p)) == E_INVALID
    rp.render(); rp.resolve_sky()
    assert np.array_equal(_bits(rp.read_sky()), _bits(want))
    rp.close()


@pytest.mark.parametrize("n", [1, 13])
def test_the_smallest_grids(ctx, n):
    assert B.star_grid_size(n) == (1 if n == 1 else 2)
    f = S.tie_frame()
    pts = [(2 + (k % 5), 2 + (k // 5)) for k in range(n)]
    got, add, st = _image(ctx, f, S.tie_stars(pts))
    assert int((add[..., 3] > 0).sum()) == n


# ---- 5.: the display pass -----------------------------------------------------------------------------------------------------------------------------------------
def test_display_is_post_ref_of_the_starred_sky_image():
    rp = _rp("single", stars=catalogue())
    rp.render()
    rp.resolve_display()                                                         # runs the sky pass, and the stars behind it, itself
    sky, disp, frame = rp.read_sky(), rp.read_display(), rp.read_hdr()
    assert np.array_equal(disp, P.post_ref(sky))
    rp.set_stars(None); rp.resolve_sky()                                         # (a sky image the frame already has is as the catalogue of its resolve made it)
    add, st = S.resolve(frame, catalogue())
    assert S.floors(st)["lit"] >= 10
    _same(sky, S.apply(rp.read_sky(), add), "display's sky pass")
    rp.close()


# ---- 6.: refusals and untouched paths -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_ctx_that_splits_the_frame():
    L = B.lib()
    cat = catalogue()
    for kw in (dict(devices=[0, 0], stripe_rows=9), dict(row_rank=0, row_world=2)):
        rp = B.RayPass(_cfg("window"), **kw)
        rp.set_textures(*T.textures())
        rp.set_uniforms(*T.uniforms(integration_method=1))
        assert L.bhray_set_stars(rp._h, cat.ctypes.data, len(cat), None) == E_STATE
        assert L.bhray_set_stars(rp._h, None, 0, None) == 0 and L.bhray_set_stars(rp._h, cat.ctypes.data, 0, None) == 0
        bad = cat.copy(); bad[0, 0] = np.nan
        assert L.bhray_set_stars(rp._h, bad.ctypes.data, len(bad), None) == E_INVALID
        rp.render(); rp.resolve_sky()
        assert rp.read_sky().shape[1] == 40                                      # the ctx keeps working
        rp.close()


def test_hdr_ray_lists_and_the_accumulation_keep_their_bits():
    from bhusie_amd import cameras
    rays = cameras.pinhole_rays(B.Camera(), 40, 36)
    out = []
    for stars in (None, catalogue()):
        rp = _rp("window", stars=stars)
        rp.render(); rp.resolve_sky()
        hdr = rp.read_hdr()
        res, sky16 = rp.trace_rays(rays, sky=True)
        rp.accum_begin(); rp.accum_add(3)
        out.append((hdr, res.copy(), sky16.copy(), rp.accum_read()))
        rp.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    assert np.array_equal(_bits(out[0][2]), _bits(out[1][2]))
    assert np.array_equal(out[0][3].view(np.uint32), out[1][3].view(np.uint32))


# ---- 7.: the hosts ------------------------------------------------------------------------------------------------------------------------------------------------
def test_renderer_set_stars_is_the_ray_pass_call():
    r = B.Renderer(_cfg("single"), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    assert r.stars is None
    r.set_stars(catalogue())
    assert np.array_equal(r.stars, catalogue())
    r.render()
    r.ray_pass.resolve_sky()
    got, frame = r.ray_pass.read_sky(), r.read_hdr()
    with pytest.raises(B.BhrayError):
        bad = catalogue().copy(); bad[0, 3] = np.inf
        r.set_stars(bad)
    assert np.array_equal(r.stars, catalogue())
    r.set_stars(None)
    assert r.stars is None
    r.ray_pass.resolve_sky()
    _same(got, S.apply(r.ray_pass.read_sky(), S.resolve(frame, catalogue())[0]), "Renderer")
    r.ray_pass.close()


def test_cpp_host_stars_seeded_flag(tmp_path):
    """bhray_render --handoff ... --stars-seeded 2000 SEED: its sky frames are the restatement of assets.star_catalogue(2000, SEED) over the same program's HDR frames
    and starless sky frames, and its display frames post_ref of its sky frames."""
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")

    def run(form, px, *extra):
        out = tmp_path / f"{form}{len(extra)}.bin"
        r = subprocess.run([exe, "--handoff", form, "2", str(out), "--rk", "--base", "24", "14", "--levels", "2", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        w, h = (int(v) for v in r.stdout.split()[0].split("x"))
        return np.fromfile(out, dtype=np.uint8).reshape(2, h, w, px)

    flag = ("--stars-seeded", "2000", str(SEED))
    sky_on = run("sky", 8, *flag).view(np.float16)
    sky_off = run("sky", 8).view(np.float16)
    hdr = run("hdr", 16).view(np.float32)
    disp_on = run("display", 4, *flag)
    for i in range(2):
        add, st = S.resolve(hdr[i], catalogue())
        assert S.floors(st)["lit"] >= 20
        _same(sky_on[i], S.apply(sky_off[i], add), f"frame {i}")
        assert np.array_equal(disp_on[i], P.post_ref(sky_on[i])), i
