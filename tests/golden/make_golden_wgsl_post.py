#!/usr/bin/env python3
"""Generates tests/golden/wgsl_exec_post.npz: the display pass (bloom x10, mix, hdr, FXAA) produced by EXECUTING THE
REFERENCE'S OWN SHADER TEXT (bloom_down / bloom_up / mix / hdr / fxaa.wgsl, parsed and run by oracle/wgsl_exec_post.py) - not by any
restatement of it.

Runs only where the reference tree exists (the build container).  What is committed is data: seeds, input images, uniform bytes, the
targets of the passes and statement hit counts (token indices and numbers) - no shader text, no file name and no line of the reference.

  (a) executed-pipeline frames: the `.sky` images of rk_ladder and rk_outside in wgsl_exec.npz (read from there, not copied); the third,
      euler_mesh_near, is 34 x 19 - under the 32 x 32 minimum - so its scene is rendered again at one level of 47 x 33 by the executed ray
      and sky shaders (`mesh47`); and `direct45`, a scene whose executed frame holds only direction pixels and the horizon's constant
      (0, 0, 0, 1) (the disk inside the unit horizon sphere, the camera inside the relativity sphere), for the GPU test that has no
      restatement in its chain.  Default uniforms.
  (b) six seeded synthetic RGBA16F images, 32x32 ... 131x70 (SYNTH below), default uniforms.
  (c) the eight uniform rows of tests/test_gpu_display.py::test_post_uniforms on the 96x54 image of (b).
Stored per case: the FXAA target as f32 and the RGBA8 image always; the ten bloom levels, mix and hdr for the small cases and where
a uniform changes them (the two large executed frames keep hdr only: the fixture must stay under the size of the largest one committed).

The generator asserts, and stores under `cov.*`, that over the whole fixture every statement of every function of the five files ran,
every `if` and loop condition came out both ways, every scalar `select` chose both ways, and that at least 1 000 FXAA fragments passed
the early exit.  If an input set misses one, change the inputs - not the condition.

FROZEN FIXTURE: regenerate only if the reference's shaders or the rules of wgsl_exec_post.py's header change, and say so in the commit.

    python tests/golden/make_golden_wgsl_post.py [--processes 16]

Wall time where the fixture was made (16 processes): 97 s, 67 s of it the two scenes of (a) that ray.wgsl is executed for.
"""
import argparse
import os
import struct
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import host_oracle as H  # noqa: E402
from oracle import wgsl_exec as W  # noqa: E402
from oracle import wgsl_exec_post as WP  # noqa: E402

# (name, W, H, seed)
SYNTH = [("s32x32", 32, 32, 3201), ("s33x32", 33, 32, 3302), ("s32x47", 32, 47, 3247), ("s63x35", 63, 35, 6335), ("s96x54", 96, 54, 9654),
         ("s131x70", 131, 70, 13170)]
# tests/test_gpu_display.py::test_post_uniforms
VARIANTS = [("low", (0.0833, 0.250, 12, 0.75), 0.7), ("extreme", (0.0078, 0.031, 12, 0.75), 0.7), ("it1", (0.0078, 0.031, 1, 0.75), 0.7),
            ("it2", (0.0078, 0.031, 2, 0.75), 0.7), ("it6", (0.0078, 0.031, 6, 1.0), 0.7), ("it20", (0.0078, 0.031, 20, 0.5), 0.7),
            ("mix0", (0.0156, 0.063, 12, 0.75), 0.0), ("mix1", (0.0156, 0.063, 12, 0.75), 1.0)]
FULL = {"s32x32", "s33x32", "s32x47", "s63x35", "s96x54", "mesh47", "direct45"}     # every target stored
SUBNORMAL = 2.0 ** -24                                                                # the smallest binary16 denormal


HDR_PEAKS = {"s63x35"}       # bloom spreads a 6.0e4 texel over the whole of a small frame and ACES then saturates all of it: one frame has them


def synth(w, h, seed, peaks=False):
    """A seeded RGBA16F image, finite everywhere.  Every image holds: star-field noise; hard edges through the frame centre in all four
    orientations, running out to the borders; an edge along each border; one-pixel lines; a checkerboard; a long edge of low slope in
    each direction (long FXAA searches); binary16 denormals; negative channels; alpha 0, 0.25 and -1.  peaks: values of 6.0e4 beside zeros
    (a single texel, and a block whose bloom sums approach the binary16 maximum) - elsewhere the brightest texels are stars of up to ~40."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    img = np.zeros((h, w, 4), np.float64)
    tint = rng.uniform(0.5, 1.0, size=3)
    # eight sectors about the centre, alternately dim and bright: horizontal, vertical and both diagonal edges through the centre
    sector = np.floor((np.arctan2(yy - cy, xx - cx) + np.pi) / (np.pi / 4.0) + 1e-9).astype(int) % 8
    img[..., :3] = np.where(sector[..., None] % 2 == 0, 0.02, 0.55) * tint
    # a long edge of low slope in each direction, offset from the centre, with its own pair of levels
    slope = rng.uniform(0.02, 0.05)
    band = (yy > cy + h * 0.22 + slope * (xx - cx)) & (yy < cy + h * 0.22 + slope * (xx - cx) + max(3, h // 8))
    img[band, :3] = rng.uniform(0.7, 1.4, size=3)
    band = (xx > cx - w * 0.3 + slope * (yy - cy)) & (xx < cx - w * 0.3 + slope * (yy - cy) + max(3, w // 10))
    img[band, :3] = rng.uniform(0.2, 0.4, size=3)
    # a checkerboard, one-pixel lines (horizontal, vertical, diagonal)
    q = (slice(h // 8, h // 8 + max(6, h // 5)), slice(w - w // 8 - max(6, w // 5), w - w // 8))
    img[q[0], q[1], :3] = (((yy + xx) % 2)[q[0], q[1]] * 0.9)[..., None]
    img[h // 3, w // 6: w // 2, :3] = (1.5, 0.1, 0.1)
    img[h // 2: h - 3, w // 4, :3] = (0.1, 1.2, 0.1)
    d = np.arange(min(w, h) // 3)
    img[h // 8 + d, w // 10 + d, :3] = (0.2, 0.2, 2.0)
    # an edge along each border: the outermost row / column differs from its neighbour over part of its length
    img[0, w // 5: w - w // 4, :3] = 0.9
    img[h - 1, w // 3: w - w // 6, :3] = (0.0, 0.8, 0.4)
    img[h // 4: h - h // 3, 0, :3] = (0.8, 0.0, 0.3)
    img[h // 5: h - h // 5, w - 1, :3] = 1.1
    # star-field noise: mostly dark, a few bright points, some of them very bright
    stars = rng.random((h, w)) < 0.04
    img[stars, :3] += (rng.random((int(stars.sum()), 1)) ** 6 * 40.0) * rng.uniform(0.6, 1.0, size=(int(stars.sum()), 3))
    # HDR values up to 6.0e4 beside zeros
    by, bx = int(h * 0.7), int(w * 0.75)
    img[by - 2: by + 3, bx - 2: bx + 3, :3] = 0.0
    img[by, bx, :3] = 6.0e4 if peaks else 30.0
    img[by - 1, bx + 1, :3] = (6.0e4, 0.0, 3.0e4) if peaks else (25.0, 0.0, 12.0)
    if peaks:
        img[by - 6: by - 2, bx - 10: bx - 2, :3] = 6.0e4
    # binary16 denormals and negative channels
    py, px = int(h * 0.55), int(w * 0.08)
    img[py: py + 3, px: px + 4, :3] = SUBNORMAL * rng.integers(1, 1000, size=(3, 4, 3))
    img[py + 4: py + 7, px: px + 4, :3] = -rng.uniform(0.01, 2.0, size=(3, 4, 3))
    img[py + 4, px + 1, :3] = (-3.0, 0.5, -0.25)
    # alpha
    img[..., 3] = 1.0
    ay, ax = int(h * 0.15), int(w * 0.45)
    img[ay: ay + 3, ax: ax + 3, 3] = 0.0
    img[ay + 3: ay + 6, ax: ax + 3, 3] = 0.25
    img[ay: ay + 6, ax + 3: ax + 6, 3] = -1.0
    img[ay: ay + 6, ax + 3: ax + 6, :3] = 0.0                 # as render_rays delivers untraced fisheye pixels
    out = img.astype(np.float16)
    assert np.isfinite(out).all()
    return out


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def executed_frame(g, cam, bh, det, size, mesh, processes):
    tex = (g["t_temp"], g["t_disk"], g["t_sky"])
    models = []
    if mesh:
        models = [dict(position=tuple(float(v) for v in g["mesh.position"]), visible=1, points=g["mesh.points"], normals=g["mesh.normals"],
                       triangles=g["mesh.triangles"], nodes=g["mesh.nodes"], bvh_lookup=g["mesh.bvh_lookup"])]
    W.compile_shader()
    frame = W.render_ladder(cam, bh, det, tex, [size], models=models, processes=processes)[0]
    assert not np.isnan(frame).any()
    return frame, W.render_sky(frame, g["t_sky"])


def store(out, name, r, full, keep_hdr=True):
    for k in ("fxaa", "rgba8"):
        out[f"{name}.{k}"] = r[k]
    if full:
        for i, l in enumerate(r["levels"]):
            out[f"{name}.level{i}"] = l.view(np.uint16)
        out[f"{name}.mix"] = r["mix"].view(np.uint16)
    if full or keep_hdr:
        out[f"{name}.hdr"] = r["hdr"].view(np.uint16)
    for k in ("mix", "hdr", "fxaa"):
        assert np.isfinite(r[k].astype(np.float32)).all(), (name, k)
    assert all(np.isfinite(l.astype(np.float32)).all() for l in r["levels"]), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=min(16, os.cpu_count() or 8))
    args = ap.parse_args()
    t_start = time.time()
    g = np.load(os.path.join(HERE, "wgsl_exec.npz"))
    pl = WP.pipeline()
    out = {}
    run = lambda sky, f=WP.FXAA_DEFAULT, m=WP.MIX_DEFAULT: pl.render_post(sky, f, m, processes=args.processes)   # noqa: E731

    def default_uniforms(name):
        out[f"{name}.fxaa_details"], out[f"{name}.mix_details"] = u8(WP.FXAA_DEFAULT), u8(WP.MIX_DEFAULT)

    # ---- (a)
    for name in ("rk_ladder", "rk_outside"):
        t0 = time.time()
        sky = g[f"{name}.sky"]
        assert min(sky.shape[:2]) >= 32
        store(out, name, run(sky), full=False)
        default_uniforms(name)
        print(f"{name}: {sky.shape[1]}x{sky.shape[0]} {time.time() - t0:.0f} s", flush=True)
    assert min(g["euler_mesh_near.sky"].shape[:2]) < 32                       # why that case is re-rendered
    scenes = {
        "mesh47": (g["euler_mesh_near.camera"].tobytes(), g["euler_mesh_near.black_hole"].tobytes(), g["euler_mesh_near.details"].tobytes(), (47, 33), True),
        "direct45": (H.camera_uniform(), H.black_hole_uniform(accretion_disk_inner=0.2, accretion_disk_outer=0.5),
                     H.ray_details(integration_method=1), (45, 34), False),
    }
    for name, (cam, bh, det, size, mesh) in scenes.items():
        t0 = time.time()
        frame, sky = executed_frame(g, cam, bh, det, size, mesh, args.processes)
        out[f"{name}.camera"], out[f"{name}.black_hole"], out[f"{name}.details"] = u8(cam), u8(bh), u8(det)
        out[f"{name}.size"] = np.array(size, np.int32)
        out[f"{name}.sky"] = sky.view(np.uint16)
        if name == "direct45":
            horizon = (frame == np.array([0, 0, 0, 1], np.float32)).all(axis=-1)
            direction = frame[..., 3] == 0
            assert (horizon | direction).all() and horizon.sum() > 20 and direction.sum() > 500, "direct45: a pixel is neither a direction nor the horizon's constant"
            out[f"{name}.frame"] = frame
        store(out, name, run(sky), full=True)
        default_uniforms(name)
        print(f"{name}: {size} {time.time() - t0:.0f} s", flush=True)

    # ---- (b)
    for name, w, h, seed in SYNTH:
        t0 = time.time()
        sky = synth(w, h, seed, name in HDR_PEAKS)
        out[f"{name}.seed"] = np.array([seed], np.int64)
        out[f"{name}.sky"] = sky.view(np.uint16)
        store(out, name, run(sky), full=name in FULL)
        default_uniforms(name)
        print(f"{name}: {time.time() - t0:.0f} s", flush=True)

    # ---- (c): the input, the bloom levels (no uniform reaches them) and - but for mix0 / mix1 - mix and hdr are s96x54's
    base = synth(96, 54, 9654)
    for vname, fx, mix in VARIANTS:
        t0 = time.time()
        name = f"s96x54.{vname}"
        fb, mb = struct.pack("<ffif", *fx), struct.pack("<f", mix)
        r = run(base, fb, mb)
        assert all(np.array_equal(a, out[f"s96x54.level{i}"].view(np.float16)) for i, a in enumerate(r["levels"]))
        changed = not np.array_equal(r["hdr"].view(np.uint16), out["s96x54.hdr"])
        assert changed == vname.startswith("mix")
        out[f"{name}.fxaa"], out[f"{name}.rgba8"] = r["fxaa"], r["rgba8"]
        if changed:
            out[f"{name}.mix"], out[f"{name}.hdr"] = r["mix"].view(np.uint16), r["hdr"].view(np.uint16)
        out[f"{name}.fxaa_details"], out[f"{name}.mix_details"] = u8(fb), u8(mb)
        print(f"{name}: {time.time() - t0:.0f} s", flush=True)

    # ---- coverage
    cov = pl.coverage()
    for stage, c in cov.items():
        for k, v in c.items():
            out[f"cov.{stage}.{k}"] = v
        assert len(c["stmt_tok"]) and (c["stmt_hits"] >= 1).all(), f"{stage}: statements never run at tokens {c['stmt_tok'][c['stmt_hits'] < 1].tolist()}"
        assert (c["cond_true"] >= 1).all() and (c["cond_false"] >= 1).all(), f"{stage}: a condition came out one way only: {c}"
        assert (c["sel_true"] >= 1).all() and (c["sel_false"] >= 1).all(), f"{stage}: a select chose one way only: {c}"
    passed = pl.first_condition_false()
    out["fxaa_past_early_exit"] = np.array([passed], np.int64)
    assert passed >= 1000, passed
    print("FXAA fragments past the early exit:", passed)

    dst = os.path.join(HERE, "wgsl_exec_post.npz")
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    print("wrote", dst, size, "bytes in", f"{time.time() - t_start:.0f} s")
    assert size <= os.path.getsize(os.path.join(HERE, "wgsl_exec.npz")), "larger than the largest committed fixture: trim stored intermediates"


if __name__ == "__main__":
    main()
