"""-m gpu: the footprint-filtered sky pass (bhray_set_sky_filter) held to tests/sky_filter_ref.py, the NumPy restatement, in every 16-bit word: the
pyramid level by level, and the pass over the device's own RGBA32F frame (read_hdr) - so nothing of the comparison depends on how the frame was traced."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from tests import common as T
from tests import post_ref as P
from tests import sky_filter_ref as S

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -5
W, H = 64, 36


def _cfg():
    return B.ladder_from_base((W, H), 3, 1)


def _rp(tex, method=1, cfg=None, filt=True, **kw):
    rp = B.RayPass(cfg if cfg is not None else _cfg(), device=0, **kw)
    rp.set_textures(*tex)
    rp.set_uniforms(*T.uniforms(integration_method=method))
    if filt:
        rp.set_sky_filter(1)
    return rp


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float16
    bad = (_bits(got) != _bits(want)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:5].tolist()}"


@functools.lru_cache(maxsize=None)
def _pyr(which):
    return S.pyramid(_sky(which))


@functools.lru_cache(maxsize=None)
def _sky(which):
    if which == "small":
        return T.textures()[2]
    if which == "odd":
        return assets.sky_texture(37, 19, seed=5)
    if which == "deep":
        return assets.sky_texture(4096, 2048, seed=2)
    if which == "tiny":
        return assets.sky_texture(64, 32, seed=2)
    raise KeyError(which)


def _tex(which):
    t = T.textures()
    return t[0], t[1], _sky(which)


def _check_pyramid(rp, which):
    pyr = _pyr(which)
    sky = _sky(which)
    sizes = B.sky_pyramid_sizes(sky.shape[1], sky.shape[0])
    assert len(sizes) == len(pyr)
    for l in range(1, len(pyr)):
        _same(rp.read_sky_pyramid_level(l, sizes[l]), pyr[l], f"{which} level {l}")
    L = B.lib()
    buf = np.zeros(4, np.uint16)
    assert L.bhray_read_sky_pyramid_level(rp._h, 0, buf.ctypes.data, sky.shape[0] * sky.shape[1]) == E_INVALID
    assert L.bhray_read_sky_pyramid_level(rp._h, len(pyr), buf.ctypes.data, 1) == E_INVALID
    assert L.bhray_read_sky_pyramid_level(rp._h, len(pyr) - 1, buf.ctypes.data, 2) == E_INVALID        # the top level holds one texel
    assert L.bhray_read_sky_pyramid_level(rp._h, len(pyr) - 1, None, 1) == E_INVALID


@pytest.mark.parametrize("which", ["small", "odd"])
def test_every_pyramid_level_is_the_restatements(which):
    rp = _rp(_tex(which))
    _check_pyramid(rp, which)
    rp.close()


def _pass(rp, which):
    """render, resolve, compare with the restatement over the device's own frame: (frame, filtered image, stats)"""
    rp.render()
    rp.resolve_sky()
    frame, got = rp.read_hdr(), rp.read_sky()
    want, st = S.resolve(frame, _sky(which), _pyr(which))
    _same(got, want, which)
    return frame, got, st


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_pass_is_the_restatement_in_every_word(method):
    rp = _rp(_tex("small"), method=method)
    frame, got, st = _pass(rp, "small")
    print({k: v for k, v in st.items() if k != "mask"})
    S.check_floors(st)
    plain, _ = S.resolve(frame, _sky("small"), _pyr("small"), enabled=False)
    assert int((_bits(got) != _bits(plain)).any(axis=-1).sum()) >= 1000
    rp.close()


def test_deep_levels():
    rp = _rp(_tex("deep"))
    _, _, st = _pass(rp, "deep")
    print({k: v for k, v in st.items() if k != "mask"})
    assert st["taps"][8] >= 25 and all(st["levels"].get(l, 0) > 0 for l in range(2, 7)), st
    rp.close()


def test_a_mostly_magnified_sky_keeps_the_unfiltered_bits():
    rp = _rp(_tex("tiny"))
    frame, got, st = _pass(rp, "tiny")
    print({k: v for k, v in st.items() if k != "mask"})
    rp.set_sky_filter(0)
    rp.resolve_sky()
    off = rp.read_sky()
    with np.errstate(invalid="ignore"):
        keep = (frame[..., 3] == 0) & ~st["mask"]
    assert int(keep.sum()) >= 1500 and st["filtered"] >= 1
    assert np.array_equal(_bits(got[keep]), _bits(off[keep]))
    colour = ~(frame[..., 3] == 0)
    assert np.array_equal(_bits(got[colour]), _bits(off[colour]))
    rp.close()


def test_off_is_off():
    tex = _tex("small")
    never = _rp(tex, filt=False, cfg=B.ladder_from_base((24, 14), 3, 2))
    never.render(); never.resolve_display()
    want_sky, want_disp = never.read_sky(), never.read_display()
    never.close()
    rp = _rp(tex, filt=True, cfg=B.ladder_from_base((24, 14), 3, 2))
    rp.render(); rp.resolve_display()
    on_sky = rp.read_sky()
    assert not np.array_equal(_bits(on_sky), _bits(want_sky))
    rp.set_sky_filter(0)
    with pytest.raises(B.BhrayError) as e:
        rp.read_sky_pyramid_level(1, (256, 128))
    assert e.value.code == E_STATE
    rp.render(); rp.resolve_display()
    assert np.array_equal(_bits(rp.read_sky()), _bits(want_sky)) and np.array_equal(rp.read_display(), want_disp)
    rp.close()


def test_toggling_between_frames_in_flight():
    tex = _tex("small")
    rp = _rp(tex, filt=False, frames_in_flight=4)
    pinned = [B.PinnedFrame(H, W, channels16=True) for _ in range(8)]
    tickets, frames, modes = [], [], []
    for i in range(8):
        mode = (i // 2) % 2                                          # off, off, on, on, off, off, on, on
        rp.set_uniforms(*T.uniforms(integration_method=1, time=0.25 * i, camera=B.Camera(position=(0.2 * i, 0.0, -19.0))))
        rp.render()
        if i % 2 == 0:
            rp.set_sky_filter(mode)                                  # between a render and its resolve: in force at that frame's resolve_sky
        rp.resolve_sky()
        tickets.append(rp.read_sky_async(pinned[i]))
        frames.append(rp.read_hdr()); modes.append(mode)
    for i in range(8):
        rp.wait_read(tickets[i])
        want, _ = S.resolve(frames[i], _sky("small"), _pyr("small"), enabled=bool(modes[i]))
        _same(pinned[i].array, want, f"frame {i} mode {modes[i]}")
    for b in pinned:
        b.free()
    rp.close()


def test_a_texture_change_rebuilds_the_pyramid():
    rp = _rp(_tex("small"))
    _pass(rp, "small")
    rp.set_texture(layouts.TEX_SKY, _sky("odd"))
    _check_pyramid(rp, "odd")
    _pass(rp, "odd")
    rp.set_texture(layouts.TEX_SKY, np.full((1, 1, 4), 90, np.uint8))       # a texture with no level above it
    with pytest.raises(B.BhrayError) as e:
        rp.read_sky_pyramid_level(1, (1, 1))
    assert e.value.code == E_INVALID
    rp.render(); rp.resolve_sky()
    want, st = S.resolve(rp.read_hdr(), np.full((1, 1, 4), 90, np.uint8))
    assert st["filtered"] == 0
    _same(rp.read_sky(), want, "1 x 1 sky")
    rp.close()


def test_display_is_post_ref_of_the_filtered_sky_image():
    cfg = B.ladder_from_base((24, 14), 3, 2)                                   # 70 x 40
    rp = _rp(_tex("small"), cfg=cfg)
    rp.render()
    rp.resolve_display()                                                       # runs the (filtered) sky pass itself
    sky = rp.read_sky()
    want, st = S.resolve(rp.read_hdr(), _sky("small"), _pyr("small"))
    assert st["filtered"] > 1000
    _same(sky, want, "display's sky pass")
    assert np.array_equal(rp.read_display(), P.post_ref(sky))
    rp.close()


@pytest.mark.parametrize("name", ["ladder3", "cropped"])
def test_ladder_and_cropped_frames(name):
    cfg = B.ladder_from_base((24, 14), 3, 3) if name == "ladder3" else B.ladder_for_frame((101, 53), 3, 2)
    if name == "cropped":
        assert (cfg.crop_x, cfg.crop_y) == (1, 1) and cfg.sizes()[-1] == (103, 55)             # the frame is a window of the last level
    rp = _rp(_tex("small"), cfg=cfg)
    _, _, st = _pass(rp, "small")
    assert st["filtered"] > 1000
    rp.close()


def test_refusals():
    tex = _tex("small")
    L = B.lib()
    for kw in (dict(devices=[0, 0], stripe_rows=9), dict(row_rank=0, row_world=2)):
        rp = B.RayPass(_cfg(), **kw)
        rp.set_textures(*tex)
        rp.set_uniforms(*T.uniforms(integration_method=1))
        assert L.bhray_set_sky_filter(rp._h, 1) == E_STATE
        assert L.bhray_set_sky_filter(rp._h, 0) == 0
        rp.render(); rp.resolve_sky()
        frame, sky = rp.read_hdr(), rp.read_sky()
        want, _ = S.resolve(frame, tex[2], enabled=False)
        _same(sky, want, f"{kw}: the ctx keeps working, unfiltered")
        rp.close()
    rp = _rp(tex, filt=False)
    assert L.bhray_set_sky_filter(rp._h, 2) == E_INVALID and L.bhray_set_sky_filter(rp._h, -1) == E_INVALID
    buf = np.zeros(256 * 128 * 4, np.uint16)
    assert L.bhray_read_sky_pyramid_level(rp._h, 1, buf.ctypes.data, 256 * 128) == E_STATE
    rp.close()


def test_ray_lists_and_the_accumulation_are_not_affected():
    from bhusie_amd import cameras
    tex = _tex("small")
    rays = cameras.pinhole_rays(B.Camera(), W, H)
    out = []
    for mode in (0, 1):
        rp = _rp(tex, filt=bool(mode))
        res, sky16 = rp.trace_rays(rays, sky=True)
        rp.accum_begin(); rp.accum_add(3)
        out.append((res.copy(), sky16.copy(), rp.accum_read()))
        rp.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    assert np.array_equal(out[0][2].view(np.uint32), out[1][2].view(np.uint32))


def test_cpp_host_sky_filter_flag(tmp_path):
    """bhray_render --handoff ... --sky-filter: the display frames are post_ref of the same program's filtered sky frames, which differ from the unfiltered ones."""
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")

    def run(form, px, *extra):
        out = tmp_path / f"{form}{len(extra)}.bin"
        r = subprocess.run([exe, "--handoff", form, "2", str(out), "--rk", "--base", "24", "14", "--levels", "2", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        w, h = (int(v) for v in r.stdout.split()[0].split("x"))
        return np.fromfile(out, dtype=np.uint8).reshape(2, h, w, px)

    sky_on = run("sky", 8, "--sky-filter").view(np.float16)
    sky_off = run("sky", 8).view(np.float16)
    disp_on = run("display", 4, "--sky-filter")
    assert not np.array_equal(_bits(sky_on), _bits(sky_off))
    for i in range(2):
        assert np.array_equal(disp_on[i], P.post_ref(sky_on[i])), i
