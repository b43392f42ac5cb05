"""NumPy restatement of the affine pose of DESIGN.md §14, written from its text (not from the C or the kernel).

apply(points, normals, m): what bhray_set_model_pose makes of a slot's rest arrays - binary32, one rounded operation at a time in the order
written: a point (x, y, z, w) becomes x' = ((m[0]*x + m[1]*y) + m[2]*z) + m[3], y' and z' with rows 1 and 2, w' = the bits of w; a normal
gets the same sums without the last addition.
from_euler(rotation, pivot, scale): the pose of bhray_pose_from_euler - the quaternion of BlackHoleUniform::update (cgmath's Euler XYZ),
"Quaternion * Vector3" applied to the three axes as the columns of R, A = R * scale, t = pivot - A pivot - in `dtype` (float32 restates the
C operation by operation up to the libm's sinf / cosf; float64 is the yardstick the C is held to)."""
from __future__ import annotations

import numpy as np

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)


def _rows(a, m, translate):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] == 4
    out = a.copy()                                                 # w: the same bytes
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    for r in range(3):
        s = m[r, 0] * x                                            # np.float32 scalar times a float32 array: one rounded product per element
        s = s + m[r, 1] * y
        s = s + m[r, 2] * z
        if translate:
            s = s + m[r, 3]
        assert s.dtype == np.float32
        out[:, r] = s
    return out


def apply(points, normals, m):
    """(posed points, posed normals) of (n, 4) float32 rest arrays under the row-major 3x4 pose m"""
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(3, 4)
    with np.errstate(all="ignore"):
        return _rows(points, m, True), _rows(normals, m, False)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def from_euler(rotation, pivot=(0.0, 0.0, 0.0), scale=1.0, dtype=np.float32):
    """(3, 4) array of `dtype`: [A | t]"""
    f = dtype
    rot, piv, scale = [f(v) for v in rotation], [f(v) for v in pivot], f(scale)
    half = f(0.5)
    sx, cx = np.sin(rot[0] * half), np.cos(rot[0] * half)
    sy, cy = np.sin(rot[1] * half), np.cos(rot[1] * half)
    sz, cz = np.sin(rot[2] * half), np.cos(rot[2] * half)
    qs = ((-sx * sy) * sz) + ((cx * cy) * cz)
    qv = [((sx * cy) * cz) + ((sy * sz) * cx), ((-sx * sz) * cy) + ((sy * cx) * cz), ((sx * sy) * cz) + ((sz * cx) * cy)]
    m = np.zeros((3, 4), dtype=f)
    for col in range(3):
        vec = [f(1.0 if k == col else 0.0) for k in range(3)]
        c = _cross(qv, vec)
        tmp = [c[k] + vec[k] * qs for k in range(3)]               # tmp = v x vec + vec * s
        c2 = _cross(qv, tmp)
        r = [c2[k] * f(2.0) + vec[k] for k in range(3)]            # (v x tmp) * 2 + vec
        for k in range(3):
            m[k, col] = r[k] * scale
    for k in range(3):
        ap = (m[k, 0] * piv[0] + m[k, 1] * piv[1]) + m[k, 2] * piv[2]
        m[k, 3] = piv[k] - ap
    assert m.dtype == f
    return m
