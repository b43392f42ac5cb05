#!/usr/bin/env python3
"""Generates tests/golden/multimodel.npz: scenes with SEVERAL models, frames produced by EXECUTING THE REFERENCE'S OWN SHADER TEXT
(ray.wgsl, parsed and run by oracle/wgsl_exec.py) with its model loop (ray.wgsl:377-389) over model_count entries.

The reference declares MAX_MODELS = 1 (ray.wgsl:2) only as the length of its fixed-capacity model array; the interpreter binds as many
models as the scene has, so these frames are the shader's text with that constant raised - the contract of BHRAY_MAX_MODELS (bhray.h).
Every model is a seeded sphere of bhusie_amd.assets.sphere_mesh_obj; what is committed is data only: the uniform bytes, the small
textures, the mesh parameters, each slot's seed (-1: a slot never uploaded), position and visibility, and the frames.  Meshes are
rebuilt from the seeds by whoever reads the file.  Every mesh stands outside the relativity sphere (radius 20): the shader tests meshes
in flat space only.  The frames are in the literal evaluation (wgsl_exec.py's header), comparable bit for bit with oracle/ray_oracle.c
under oracle_set_eval(1) and the BHRAY_F_LITERAL kernel.

Runs only where the reference's shader is present.  FROZEN FIXTURE: regenerate only if the shader or the literal conventions change.

    python tests/golden/make_golden_multimodel.py [--processes 8]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from bhusie_amd import assets  # noqa: E402
from oracle import host_oracle as H  # noqa: E402

MESH = dict(n_lat=8, n_lon=10, radius=12.0, bump=0.2)        # ~140 triangles per sphere
CAMERA = dict(position=(0.0, 0.0, -90.0), forward=(0.0, 0.0, 1.0), fov=0.7)
A, A2, B_, C_ = (-30.0, 0.0, 0.0), (-27.0, 1.0, -3.0), (30.0, 2.0, 5.0), (0.0, -28.0, 0.0)
# name: (details, base, levels, [(seed or -1, position, visible)] one entry per slot below model_count)
SCENES = {
    "rk_pair": (dict(integration_method=1), (16, 9), 2, [(3, A, 1), (5, A2, 1)]),                          # two overlapping spheres
    "euler_four": (dict(integration_method=0), (16, 9), 2, [(3, A, 1), (5, A2, 1), (7, B_, 1), (9, C_, 1)]),
    "rk_holes": (dict(integration_method=1), (16, 9), 3, [(7, B_, 1), (5, A2, 0), (-1, (0.0, 0.0, 0.0), 0), (3, A, 1)]),   # invisible, never uploaded
    "euler_three": (dict(integration_method=0, time=1.5), (16, 9), 3, [(9, C_, 1), (3, A, 1), (5, A2, 1)]),
}


def mesh_obj(seed):
    return assets.sphere_mesh_obj(MESH["n_lat"], MESH["n_lon"], radius=MESH["radius"], bump=MESH["bump"], seed=int(seed), with_normals=True)


def oracle_models(slots):
    """The oracles' model list (one dict per slot below model_count) from (seed, position, visible) slots: a slot never uploaded is a
    default ModelUniform (visible 0, no triangles: triangle.rs:297)."""
    out = []
    for seed, pos, vis in slots:
        if seed < 0:
            out.append(dict(position=(0.0, 0.0, 0.0), visible=0, points=np.zeros((0, 4), np.float32), normals=np.zeros((0, 4), np.float32),
                            triangles=np.zeros((0, 6), np.int32), nodes=np.zeros(32, np.uint8), bvh_lookup=np.zeros(0, np.int32)))
            continue
        m = H.load_model(mesh_obj(seed)).as_oracle_dict()
        m["position"] = tuple(float(v) for v in pos); m["visible"] = int(vis)
        out.append(m)
    return out


def ladder(base, levels):
    sizes = [tuple(base)]
    for _ in range(levels - 1):
        sizes.append((sizes[-1][0] * 3 - 2, sizes[-1][1] * 3 - 2))
    return sizes


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def main():
    from oracle import wgsl_exec as W
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=os.cpu_count() or 8)
    args = ap.parse_args()
    W.compile_shader()                                        # parse once, before the pool forks
    tex = (assets.temp_lut(32), assets.disk_texture(96, seed=11), assets.sky_texture(128, 64, seed=12))
    out = dict(t_temp=tex[0], t_disk=tex[1], t_sky=tex[2],
               mesh_params=np.array([MESH["n_lat"], MESH["n_lon"]], np.int32), mesh_shape=np.array([MESH["radius"], MESH["bump"]], np.float64))
    for name, (dk, base, levels, slots) in SCENES.items():
        cam, bh = H.camera_uniform(**CAMERA), H.black_hole_uniform()
        det = H.ray_details(model_count=len(slots), **dk)
        sizes = ladder(base, levels)
        t0 = time.time()
        imgs = W.render_ladder(cam, bh, det, tex, sizes, models=oracle_models(slots), processes=args.processes)
        out[f"{name}.camera"] = u8(cam); out[f"{name}.black_hole"] = u8(bh); out[f"{name}.details"] = u8(det)
        out[f"{name}.sizes"] = np.array(sizes, dtype=np.int32)
        out[f"{name}.seeds"] = np.array([s[0] for s in slots], np.int32)
        out[f"{name}.positions"] = np.array([s[1] for s in slots], np.float32)
        out[f"{name}.visible"] = np.array([s[2] for s in slots], np.int32)
        for l, im in enumerate(imgs):
            assert not np.isnan(im[..., 3]).any(), "a pixel was not stored"
            out[f"{name}.level{l}"] = im
        print(f"{name}: {sizes} {time.time() - t0:.0f} s", flush=True)
    dst = os.path.join(HERE, "multimodel.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
