"""Shared by tests/test_gpu_trace_rays.py and tests/test_trace_rays_host.py: the seeded ray list of the arbitrary-origin comparison and its oracle results (oracle.trace_ray
per ray), computed once per (method, mesh) and never modified."""
from __future__ import annotations

import functools

import numpy as np

import bhusie_amd as B
from bhusie_amd import assets
from oracle import oracle as O
from tests import common as T

N_RAYS = 4133              # not a multiple of 64: the host variant pads nothing
SEED = 20240611
HOLE = (0.0, 0.0, 0.0)
R_SPHERE = 20.0            # BlackHole().relativity_sphere_radius
MESH_POS = (-16.0, 4.0, 26.0)
MIN_PER_CLASS = 300


def _normalize32(v):
    """the binary32 normalise the kernels expect: v * (1 / sqrt((x*x + y*y) + z*z))"""
    v = v.astype(np.float32)
    d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return (v * (np.float32(1.0) / np.sqrt(d, dtype=np.float32))[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def seeded_rays(n=N_RAYS, seed=SEED, hole=HOLE):
    """(n, 8) float32 records.  Origins alternate by index between inside (even) and outside (odd) the relativity sphere - every wave starts in both modes -, 3 to 60 from
    the hole; every ray aims at a point of the disc of radius 12 through the hole, perpendicular to the line from the origin to the hole, so that it ends in the horizon,
    on the accretion disk or escapes."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    inside = (i % 2) == 0
    dist = np.where(inside, rng.uniform(3.0, R_SPHERE - 0.5, n), rng.uniform(R_SPHERE + 0.5, 60.0, n))
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    origin = np.asarray(hole)[None, :] + dist[:, None] * u
    a = np.cross(u, np.where(np.abs(u[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])); a /= np.linalg.norm(a, axis=1)[:, None]
    b = np.cross(u, a)
    rad, phi = 12.0 * rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 2.0 * np.pi, n)       # (denser towards the hole: enough rays for the horizon)
    target = np.asarray(hole)[None, :] + rad[:, None] * (np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b)
    rec = np.zeros((n, 8), dtype=np.float32)
    rec[:, 0:3] = origin.astype(np.float32)
    rec[:, 4:7] = _normalize32(target - rec[:, 0:3].astype(np.float64))
    rec.setflags(write=False)
    return rec


def scene_uniforms(method, model_count=0):
    return T.uniforms(black_hole=B.BlackHole(position=HOLE), integration_method=method, model_count=model_count)


@functools.lru_cache(maxsize=None)
def mesh_path():
    import os
    import tempfile
    p = os.path.join(tempfile.mkdtemp(prefix="bhray_rays_"), "sphere.obj")
    with open(p, "w") as f:
        f.write(assets.sphere_mesh_obj(10, 12, radius=11.0, bump=0.2, seed=4, with_normals=True))       # a few hundred triangles
    return p


def mesh_model(pos=MESH_POS):
    m = B.load_model(mesh_path())
    m.set_transform(pos, 1)
    return m


def oracle_rays(scene, rec):
    """oracle.trace_ray per record -> (results (n, 4), disk_hits per ray)"""
    out = np.zeros((rec.shape[0], 4), dtype=np.float32)
    disk = np.zeros(rec.shape[0], dtype=np.int64)
    cnt = O.Counters()
    before = 0
    for k in range(rec.shape[0]):
        out[k] = O.trace_ray(scene, rec[k, [0, 1, 2, 4, 5, 6]], cnt)
        disk[k] = int(cnt.disk_hits) - before
        before = int(cnt.disk_hits)
    return out, disk


@functools.lru_cache(maxsize=None)
def reference(method, mesh=False):
    """(records, oracle results, disk hits per ray) of the seeded list under scene_uniforms(method); mesh: with mesh_model() in slot 0"""
    rec = seeded_rays()
    models = [mesh_model().arrays()] if mesh else []
    sc = T.oracle_scene(*scene_uniforms(method, 1 if mesh else 0), T.textures(), models)
    want, disk = oracle_rays(sc, rec)
    want.setflags(write=False); disk.setflags(write=False)
    return rec, want, disk


def class_counts(rec, want, disk, hole=HOLE):
    """rays per outcome: a disk contribution, the horizon (opaque black, no disk), an escape (alpha 0) from inside / from outside the sphere"""
    d = rec[:, 0:3].astype(np.float64) - np.asarray(hole)[None, :]
    inside = np.sqrt((d * d).sum(axis=1)) < R_SPHERE
    esc = want[:, 3] == 0.0
    return {"disk": int((disk > 0).sum()), "horizon": int(((want[:, 3] == 1.0) & (disk == 0) & (want[:, :3] == 0.0).all(axis=1)).sum()),
            "escape_inside": int((esc & inside).sum()), "escape_outside": int((esc & ~inside).sum())}
