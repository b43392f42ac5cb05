"""CPU: bhusie_amd/cameras.py - pinhole_rays is the shader's create_ray bit for bit (the oracle's), equirect_rays and fisheye_rays against a float64 closed form."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras
from oracle import oracle as O
from tests import common as T

CAMERAS = [B.Camera(), B.Camera(position=(1.0, 2.0, -19.0), forward=(0.1, -0.2, 1.0), fov=1.1), B.Camera(position=(-30.0, 4.0, 7.0), forward=(0.8, 0.1, -0.3), fov=0.6)]
POSITION = (4.0, -3.0, -26.0)
FORWARDS = [(0.0, 0.0, 1.0), (0.3, -0.2, 0.9), (-0.7, 0.1, -0.4)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _basis64(forward):
    """create_ray's basis in float64: plane_up = (0, -1, 0)"""
    f = np.asarray(forward, dtype=np.float32).astype(np.float64)
    right = np.cross(f, [0.0, -1.0, 0.0]); right /= np.linalg.norm(right)
    up = np.cross(f, right); up /= np.linalg.norm(up)
    return f / np.linalg.norm(f), right, up


def _ulps_from_unit(d):
    """|length - 1| in units of 2^-23 (an ulp of 1)"""
    n = np.sqrt((d.astype(np.float64) ** 2).sum(axis=-1))
    return np.abs(n - 1.0) / 2.0 ** -23


@pytest.mark.parametrize("size", [(96, 54), (55, 97)])
@pytest.mark.parametrize("cam", range(len(CAMERAS)))
def test_pinhole_rays_are_create_ray_bit_for_bit(cam, size):
    w, h = size
    camera = CAMERAS[cam]
    sc = T.oracle_scene(*T.uniforms(camera=camera), T.textures())
    want = np.zeros((h, w, 6), dtype=np.float32)
    packed, keep = sc._pack()                                     # oracle.create_ray, with the scene packed once for the whole grid
    create = O.lib().oracle_create_ray
    for y in range(h):
        for x in range(w):
            create(C.byref(packed), x, y, w, h, want[y, x].ctypes.data)
    assert np.array_equal(_bits(want[h // 3, w // 4]), _bits(O.create_ray(sc, w // 4, h // 3, w, h)))
    got = cameras.pinhole_rays(camera, w, h)
    assert got.shape == (h * w, 8) and got.dtype == np.float32 and not got[:, 3].any() and not got[:, 7].any()
    got = got.reshape(h, w, 8)
    assert np.array_equal(_bits(got[..., 0:3]), _bits(want[..., 0:3])), "origins"
    differ = int((_bits(got[..., 4:7]) != _bits(want[..., 3:6])).any(axis=2).sum())
    assert differ == 0, f"{differ} of {w * h} directions differ from oracle.create_ray"
    assert np.array_equal(_bits(cameras.pinhole_rays(camera.uniform(), w, h)), _bits(got.reshape(-1, 8))), "the uniform's 32 bytes are the same camera"


@pytest.mark.parametrize("size", [(64, 32), (33, 17), (7, 5)])
@pytest.mark.parametrize("forward", FORWARDS)
def test_equirect_rays(forward, size):
    w, h = size
    r = cameras.equirect_rays(POSITION, forward, w, h)
    assert r.shape == (h * w, 8) and r.dtype == np.float32
    assert np.array_equal(r[:, 0:3], np.broadcast_to(np.asarray(POSITION, np.float32), (h * w, 3)))
    d = r[:, 4:7].reshape(h, w, 3)
    assert _ulps_from_unit(d).max() <= 2.0
    f, right, up = _basis64(forward)
    lon = (np.arange(w) - (w - 1) / 2.0) * (2.0 * np.pi / w)
    lat = (np.arange(h) - (h - 1) / 2.0) * (np.pi / h)
    want = (np.cos(lat)[:, None, None] * np.cos(lon)[None, :, None]) * f + (np.cos(lat)[:, None, None] * np.sin(lon)[None, :, None]) * right + np.sin(lat)[:, None, None] * up
    assert np.abs(d - want).max() <= 1e-6
    if w % 2 == 1 and h % 2 == 1:                                 # the centre pixel looks along forward
        assert np.abs(d[h // 2, w // 2] - f).max() <= 1e-6
    assert d[0, w // 2] @ up < 0.0 < d[h - 1, w // 2] @ up        # row 0 is the top: `up` is the direction in which rows increase (create_ray)
    # left / right and up / down symmetry in the camera's basis
    comp = np.stack([d @ f, d @ right, d @ up], axis=-1)
    assert np.abs(comp[:, ::-1, 0] - comp[..., 0]).max() <= 1e-6 and np.abs(comp[:, ::-1, 1] + comp[..., 1]).max() <= 1e-6 and np.abs(comp[:, ::-1, 2] - comp[..., 2]).max() <= 1e-6
    assert np.abs(comp[::-1, :, 2] + comp[..., 2]).max() <= 1e-6 and np.abs(comp[::-1, :, 0] - comp[..., 0]).max() <= 1e-6
    if w % 2 == 0:                                                # antipodal columns: opposite in the horizontal plane, equal in height
        a, b = comp[:, : w // 2], comp[:, w // 2:]
        assert np.abs(a[..., 0] + b[..., 0]).max() <= 1e-6 and np.abs(a[..., 1] + b[..., 1]).max() <= 1e-6 and np.abs(a[..., 2] - b[..., 2]).max() <= 1e-6
        opposite = d[::-1, : w // 2] + d[:, w // 2:]              # ... and with the rows mirrored, opposite directions
        assert np.abs(opposite).max() <= 1e-6


@pytest.mark.parametrize("fov", [1.0, 3.0, 2.0 * np.pi])
@pytest.mark.parametrize("size", [(33, 33), (40, 25), (8, 9)])
@pytest.mark.parametrize("forward", FORWARDS)
def test_fisheye_rays(forward, size, fov):
    w, h = size
    r = cameras.fisheye_rays(POSITION, forward, w, h, fov)
    assert r.shape == (h * w, 8) and r.dtype == np.float32
    d = r[:, 4:7].reshape(h, w, 3)
    f, right, up = _basis64(forward)
    radius = min(w - 1, h - 1) / 2.0
    x = (np.arange(w) - (w - 1) / 2.0)[None, :] / radius
    y = (np.arange(h) - (h - 1) / 2.0)[:, None] / radius
    rr = np.sqrt(x * x + y * y)
    outside = rr > 1.0 + 1e-6
    inside = rr < 1.0 - 1e-6                                     # (a pixel exactly on the circle may round to either side)
    assert outside.any() and (d[outside] == 0.0).all(), "pixels outside the image circle have a zero direction"
    assert _ulps_from_unit(d[inside]).max() <= 2.0
    theta = rr * (fov / 2.0)
    safe = np.where(rr > 0, rr, 1.0)
    want = np.cos(theta)[..., None] * f + (np.sin(theta) * x / safe)[..., None] * right + (np.sin(theta) * y / safe)[..., None] * up
    assert np.abs(d[inside] - want[inside]).max() <= 1e-6
    if w % 2 == 1 and h % 2 == 1:
        assert np.abs(d[h // 2, w // 2] - f).max() <= 1e-6
    comp = np.stack([d @ f, d @ right, d @ up], axis=-1)
    assert np.abs(comp[:, ::-1, 1] + comp[..., 1]).max() <= 1e-6 and np.abs(comp[:, ::-1, 0] - comp[..., 0]).max() <= 1e-6     # left / right
    assert np.abs(comp[::-1, :, 2] + comp[..., 2]).max() <= 1e-6 and np.abs(comp[::-1, :, 0] - comp[..., 0]).max() <= 1e-6     # up / down
