"""CPU: bhray_pose_from_euler (host arithmetic of libbhray) against tests/pose_ref.py evaluated in float64, its known answers and argument
checks, and the properties of the restatement pose_ref.apply that tests/test_gpu_pose.py holds the pose kernel to byte for byte.

The bound: fewer than 16 rounded binary32 operations on values of size max(1, |scale|, |scale| max|pivot|) stand behind an entry of the pose,
each contributing at most 2^-24 relative (16 x 2^-24 = 0.95e-6), and the host libm's sinf / cosf may add an ulp: 2e-6 times that size."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import pose_ref as PR

E_INVALID = -1


def _bound(pivot, scale):
    return 2e-6 * max(1.0, abs(scale), abs(scale) * max(abs(float(v)) for v in pivot))


def _cases():
    rng = np.random.default_rng(20240614)
    out = [((0.3, 0.7, -0.2), (0.0, 0.0, 0.0), 1.0), ((0.15, 0.0, 0.25), (1.0, -2.0, 3.0), 1.5), ((-3.0, 2.5, 1.0), (-10.0, 0.0, 30.0), 0.25),
           ((0.0, 0.0, 0.0), (4.0, 5.0, -6.0), -2.0)]
    for _ in range(12):
        out.append((tuple(rng.uniform(-np.pi, np.pi, 3)), tuple(rng.uniform(-20.0, 20.0, 3)), float(rng.uniform(0.1, 4.0))))
    return out


@pytest.mark.parametrize("rotation,pivot,scale", _cases())
def test_pose_from_euler_against_the_restatement_in_float64(rotation, pivot, scale):
    got = B.pose_from_euler(rotation, pivot, scale)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    rot32, piv32, s32 = [np.float32(v) for v in rotation], [np.float32(v) for v in pivot], np.float32(scale)     # the inputs the C sees
    want = PR.from_euler(rot32, piv32, s32, dtype=np.float64)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"max |C - float64| = {err:.3g}, bound {_bound(pivot, scale):.3g}")
    assert err <= _bound(pivot, scale)
    # the float32 restatement is held to the same yardstick (it is what the GPU tests build their poses with)
    assert float(np.abs(PR.from_euler(rotation, pivot, scale).astype(np.float64) - want).max()) <= _bound(pivot, scale)


def test_zero_rotation_is_the_identity_exactly():
    assert np.array_equal(B.pose_from_euler((0.0, 0.0, 0.0)), PR.IDENTITY)
    assert np.array_equal(B.pose_from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0), PR.IDENTITY)
    assert np.array_equal(PR.from_euler((0.0, 0.0, 0.0)), PR.IDENTITY)


@pytest.mark.parametrize("axis,images", [
    (0, ((1, 0, 0), (0, 0, 1), (0, -1, 0))),        # the quaternion (cos 45, sin 45 (1, 0, 0)): y -> z, z -> -y
    (1, ((0, 0, -1), (0, 1, 0), (1, 0, 0))),        # about y: z -> x, x -> -z
    (2, ((0, 1, 0), (-1, 0, 0), (0, 0, 1))),        # about z: x -> y, y -> -x
])
def test_quarter_turns_map_the_axes_as_the_quaternion_convention_says(axis, images):
    rotation = [0.0, 0.0, 0.0]
    rotation[axis] = np.pi / 2
    m = B.pose_from_euler(rotation)
    want = np.array(images, dtype=np.float64).T                    # column c = the image of axis c
    assert float(np.abs(m[:, :3].astype(np.float64) - want).max()) <= _bound((0, 0, 0), 1.0)
    assert np.array_equal(m[:, 3], np.zeros(3, np.float32))
    # about a pivot on the axis nothing moves along it; a point off the axis goes round the pivot
    pivot = [0.0, 0.0, 0.0]
    pivot[(axis + 1) % 3] = 2.0
    p = B.pose_from_euler(rotation, pivot, 1.0).astype(np.float64)
    assert float(np.abs(p[:, :3] @ np.array(pivot) + p[:, 3] - np.array(pivot)).max()) <= _bound(pivot, 1.0)     # the pivot is a fixed point


def test_rotations_are_orthogonal():
    rng = np.random.default_rng(7)
    for _ in range(16):
        r = B.pose_from_euler(tuple(rng.uniform(-np.pi, np.pi, 3)))[:, :3].astype(np.float64)
        assert float(np.abs(r @ r.T - np.eye(3)).max()) <= _bound((0, 0, 0), 1.0)
        assert np.linalg.det(r) > 0.999


def test_argument_checks():
    L = B.lib()
    f3 = C.c_float * 3
    out = (C.c_float * 12)()
    ok = f3(0.1, 0.2, 0.3)
    assert L.bhray_pose_from_euler(ok, f3(0, 0, 0), 1.0, out) == 0
    assert L.bhray_pose_from_euler(ok, f3(0, 0, 0), 1.0, None) == E_INVALID
    assert L.bhray_pose_from_euler(None, f3(0, 0, 0), 1.0, out) == E_INVALID
    assert L.bhray_pose_from_euler(ok, None, 1.0, out) == E_INVALID
    assert L.bhray_pose_from_euler(f3(0.1, float("nan"), 0.3), f3(0, 0, 0), 1.0, out) == E_INVALID
    assert L.bhray_pose_from_euler(ok, f3(0, float("inf"), 0), 1.0, out) == E_INVALID
    assert L.bhray_pose_from_euler(ok, f3(0, 0, 0), float("nan"), out) == E_INVALID
    with pytest.raises(B.BhrayError) as e:
        B.pose_from_euler((float("nan"), 0.0, 0.0))
    assert e.value.code == E_INVALID


# ---- the restatement the pose kernel is compared with -------------------------------------------------------------
def _arrays():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-9.0, 9.0, (37, 4)).astype(np.float32)
    nrm = rng.uniform(-1.0, 1.0, (11, 4)).astype(np.float32)
    pts.view(np.uint32)[:, 3] = rng.integers(0, 2 ** 32, 37, dtype=np.uint64).astype(np.uint32)
    pts.view(np.uint32)[5, 3] = 0x7FC12345                         # a NaN with a payload
    nrm.view(np.uint32)[2, 3] = 0x7FC12345
    nrm.view(np.uint32)[3, 3] = 0xFF800001                         # a signalling NaN
    return pts, nrm


def test_apply_keeps_the_bits_of_w():
    pts, nrm = _arrays()
    for m in (PR.IDENTITY, PR.from_euler((0.3, 0.7, -0.2), (1.0, 2.0, 3.0), 1.5), np.zeros((3, 4), np.float32)):
        p, n = PR.apply(pts, nrm, m)
        assert np.array_equal(p.view(np.uint32)[:, 3], pts.view(np.uint32)[:, 3])
        assert np.array_equal(n.view(np.uint32)[:, 3], nrm.view(np.uint32)[:, 3])
        assert p.view(np.uint32)[5, 3] == 0x7FC12345 and n.view(np.uint32)[3, 3] == 0xFF800001
        assert np.isfinite(p[:, :3]).all() and np.isfinite(n[:, :3]).all()


def test_apply_with_the_identity_turns_minus_zero_into_plus_zero_and_changes_nothing_else():
    pts, nrm = _arrays()
    pts[4, 0] = pts[9, 1] = pts[9, 2] = pts[20, 2] = np.float32(-0.0)
    assert (pts.view(np.uint32)[:, :3] == 0x80000000).sum() == 4
    p, _ = PR.apply(pts, nrm, PR.IDENTITY)
    want = pts.copy()
    want.view(np.uint32)[:, :3][pts.view(np.uint32)[:, :3] == 0x80000000] = 0          # (.. + -0) + 0 = +0: the translation is added last
    assert np.array_equal(p.view(np.uint32), want.view(np.uint32))


def test_apply_does_not_translate_a_normal():
    pts, nrm = _arrays()
    m = PR.from_euler((0.3, 0.7, -0.2), (1.0, 2.0, 3.0), 1.5)
    moved = m.copy()
    moved[:, 3] += np.float32(5.0)
    p0, n0 = PR.apply(pts, nrm, m)
    p1, n1 = PR.apply(pts, nrm, moved)
    assert np.array_equal(n0.view(np.uint32), n1.view(np.uint32))
    assert not np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    lin = m.copy()
    lin[:, 3] = 0.0
    as_points, _ = PR.apply(nrm, nrm, lin)                         # a point under t = +0 differs from a normal only in the sign of a zero
    assert np.array_equal(n0[:, :3], as_points[:, :3])


def test_cpp_host_program_refuses_a_pose_without_the_device_builder(tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    for args in (["--pose", "0.3", "0.7", "-0.2"], ["--bvh", "reference", "--pose", "0.3", "0.7", "-0.2"]):      # a usage error, before any device is touched
        r = subprocess.run([exe, str(tmp_path / "o.f32")] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--bvh device" in r.stderr, (args, r.stderr)
    r = subprocess.run([exe, str(tmp_path / "o.f32"), "--bvh", "device", "--pose", "0.3", "0.7"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2                                       # three angles
