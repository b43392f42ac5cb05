"""CPU: the arithmetic of the accumulation image - the library's sample offsets against the NumPy restatement (tests/accum_ref.py), the properties
the header promises of them, cameras.r2_offset, and pinhole_rays' additive arguments."""
import ctypes as C

import numpy as np

import bhusie_amd as B
from bhusie_amd import cameras
from tests import accum_ref as A


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lib_offset(s):
    dx, dy = C.c_float(), C.c_float()
    B.lib().bhray_accum_sample_offset(s, C.byref(dx), C.byref(dy))
    return np.float32(dx.value), np.float32(dy.value)


def test_the_librarys_offsets_are_the_restatements():
    for s in range(4096):
        got, want = _lib_offset(s), A.offset(s)
        assert np.array_equal(_bits(got), _bits(want)), (s, got, want)
        assert np.array_equal(_bits(cameras.r2_offset(s)), _bits(want)), s
    for s in (65535, 2 ** 31, 2 ** 32 - 1):                      # the integer products wrap mod 2^32
        assert np.array_equal(_bits(_lib_offset(s)), _bits(A.offset(s))), s
    L = B.lib()
    L.bhray_accum_sample_offset(3, None, None)                    # a NULL output is not written


def test_offset_zero_is_the_pixel_centre_and_all_lie_in_the_pixel():
    assert _bits(_lib_offset(0)).tolist() == [0, 0]               # +0.0, +0.0
    off = np.array([_lib_offset(s) for s in range(4096)], dtype=np.float32)
    assert (off >= -0.5).all() and (off < 0.5).all()
    assert len({tuple(o) for o in _bits(off[:8]).tolist()}) == 8, "offsets 0-7 are distinct"
    # the first constant is round(2^32 / rho), rho the plastic number (x^3 = x + 1); the second is 2^32 / rho^2 made odd (an odd multiplier visits all 2^32 values)
    rho = 1.3247179572447460
    assert 0xC13FA9A9 == round(2 ** 32 / rho) and abs(0x91E10DA5 - 2 ** 32 / rho ** 2) < 1.0 and 0x91E10DA5 % 2 == 1
    # low discrepancy, roughly: 64 samples put 14-18 into each quadrant of the pixel
    q = ((off[:64, 0] >= 0).astype(int) * 2 + (off[:64, 1] >= 0).astype(int))
    assert np.bincount(q, minlength=4).min() >= 12


def test_pinhole_rays_defaults_keep_their_bits():
    cam = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
    plain = cameras.pinhole_rays(cam, 40, 36)
    assert np.array_equal(_bits(plain), _bits(cameras.pinhole_rays(cam, 40, 36, offset=(0, 0))))
    assert np.array_equal(_bits(plain), _bits(cameras.pinhole_rays(cam, 40, 36, offset=(0.0, 0.0), level=(40, 36), crop=(0, 0))))
    one = cameras.pinhole_rays(cam, 40, 36, pixel=(7, 5), offset=(0.0, 0.0))
    assert np.array_equal(_bits(one[0]), _bits(plain[5 * 40 + 7]))


def test_a_window_of_a_level_is_that_levels_rays():
    cam = B.Camera()
    level = cameras.pinhole_rays(cam, 46, 37).reshape(37, 46, 8)
    win = cameras.pinhole_rays(cam, 40, 36, level=(46, 37), crop=(3, 1)).reshape(36, 40, 8)
    assert np.array_equal(_bits(win), _bits(level[1:37, 3:43]))
    off = cameras.pinhole_rays(cam, 40, 36, offset=(0.25, -0.5), level=(46, 37), crop=(3, 1))
    assert np.isfinite(off).all() and not np.array_equal(_bits(off), _bits(win.reshape(-1, 8)))
    n = np.linalg.norm(off[:, 4:7].astype(np.float64), axis=1)
    assert np.abs(n - 1.0).max() < 1e-6


def test_sample_rays_of_sample_zero_on_a_cropped_ladder():
    cfg = B.ladder_for_frame((40, 36), 3, 2)
    lw, lh = cfg.sizes()[-1]
    cam = B.Camera()
    want = cameras.pinhole_rays(cam, lw, lh).reshape(lh, lw, 8)[cfg.crop_y:cfg.crop_y + 36, cfg.crop_x:cfg.crop_x + 40]
    assert np.array_equal(_bits(A.sample_rays(cam, cfg, 0)), _bits(want.reshape(-1, 8)))


def test_restated_sum_and_mean():
    sky = np.full((2, 2, 4), 255, np.uint8)                       # white: sky^4 = 1
    nan = np.float32(np.nan)
    a = np.array([[0.5, 0.25, 0.125, 1.0], [0.0, 1.0, 0.0, 0.0], [nan, 0.0, 0.0, 1.0]], np.float32)
    b = np.array([[0.25, 0.25, 0.25, 1.0], [0.1, 0.2, 0.3, 1.0], [0.0, nan, 0.0, 1.0]], np.float32)
    total = A.accumulate([a, b], sky)
    assert total.dtype == np.float32
    assert total[:, 3].tolist() == [2.0, 2.0, 0.0]
    m = A.mean(total)
    assert np.array_equal(m[0], np.array([0.375, 0.25, 0.1875, 1.0], np.float32))
    assert np.array_equal(m[1], ((np.array([1.0, 1.0, 1.0], np.float32) + np.array([0.1, 0.2, 0.3], np.float32)) / np.float32(2.0)).tolist() + [1.0])
    assert m[2].tolist() == [0.0, 0.0, 0.0, 0.0]
