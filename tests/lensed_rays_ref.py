"""Lensed meshes in ray batches and ray records (bhray_set_mesh_lensing's BHRAY_LENS_RAYS) restated in NumPy: the reference the GPU tests compare with.

`trace_rays_lensed_records` below is `tests/ray_records_ref.py::trace_rays_records` written out again with `tests/lensed_ref.py`'s per-ray model loop behind
`hit_black_hole` of the relativity branch: every visible model over the step's segment - the previous position with the NEW direction, range (t_min, step) - through
`ray_records_ref._trace_ray_model_slot`, every model with the full range, a strictly nearer hit replacing what stands (the black hole's result first, then the earlier
models'), its colour times the diffuse factor, opacity 1.  Beside the hit the loop remembers the model, the triangle and that the standing hit came from a segment.
Everything else is ray_records_ref's text, and everything it calls is np_ray's own.

Also here: the scene (four icospheres, slot 1 invisible, slot 3 straddling R = 20), the ray list - a third aimed near the hole, a third aimed at a visible mesh from
inside the sphere, a third from outside -, the references computed once per process, and the figures the lists are held to on the reference alone.
"""
from __future__ import annotations

import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

import bhusie_amd as B
from bhusie_amd import assets, RAY_RECORD_DTYPE, HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH
from oracle import np_ray as N
from tests import lensed_ref as LR
from tests import ray_records_ref as RRR
from tests import rays_ref as RR

f32 = np.float32

# (radius, position, visible) of an 80-triangle icosphere per slot
SLOTS = [(3, (3.5, -1.5, -8.0), 1), (4, (0.0, 6.0, 0.0), 0), (7, (0.5, 2.0, 11.0), 1), (8, (-10.0, 0.0, 17.0), 1)]
N_RAYS = 1003               # not a multiple of 64
N_RAYS_CPU = 259            # the CPU test's list
SEED = 20241021


def trace_rays_lensed_records(S: N.Scene, origin, direction):
    """-> (results (n, 4) float32 - lensed_ref.trace_rays_lensed's -, records (n,) RAY_RECORD_DTYPE, margin (n,) float32 - ray_records_ref's rule -, seg_first (n,) bool:
    the first accepted hit was a segment's mesh hit, stats: segment_hits - segments a model won -, segment_hits_after_disk - those on a ray that had hit before)"""
    n = origin.shape[0]
    t_max, t_min = f32(1e5), f32(1e-8)
    cpos, cdir = origin.copy(), direction.copy()
    ppos, pdir = origin.copy(), direction.copy()
    rkpos, rkdir = origin.copy(), direction.copy()
    rkh = np.full(n, S.step_size, dtype=np.float32)
    ray_distance = N.vlen(origin - S.bh_pos)
    rel = ray_distance < S.R
    amount = np.ones(n, dtype=np.float32)
    color = np.zeros((n, 3), dtype=np.float32)
    step = np.full(n, S.step_size, dtype=np.float32)
    hit = np.zeros(n, dtype=bool)
    closest = N.vlen(cpos - S.bh_pos)
    alive = np.ones(n, dtype=bool)
    i_final = np.full(n, S.max_iter, dtype=np.int64)
    # ---- the records' bookkeeping
    rec = np.zeros(n, dtype=RAY_RECORD_DTYPE)
    rec["hit"] = HIT_NONE; rec["triangle"] = -1
    margin = np.full(n, np.abs(f32(1.0) - f32(0.005)), dtype=np.float32)
    seg_first = np.zeros(n, dtype=bool)
    segment_hits = 0
    segment_hits_after_disk = 0
    light = LR._light()
    for it in range(S.max_iter):
        if not alive.any():
            break
        c_hit = np.zeros(n, dtype=bool); c_t = np.zeros(n, dtype=np.float32)
        c_col = np.zeros((n, 3), dtype=np.float32); c_op = np.zeros(n, dtype=np.float32)
        c_kind = np.zeros(n, dtype=np.uint32); c_model = np.zeros(n, dtype=np.int64); c_tri = np.full(n, -1, dtype=np.int64)
        c_seg = np.zeros(n, dtype=bool)
        kr = np.nonzero(alive & rel)[0]
        kf = np.nonzero(alive & ~rel)[0]
        if kr.size:
            ppos[kr] = cpos[kr]; pdir[kr] = cdir[kr]
            if S.method == 0:
                np_, nd_ = N.next_ray_euler(S, cpos[kr], cdir[kr], step[kr])
                cpos[kr] = np_; cdir[kr] = nd_
            else:
                np_, nd_, nh_ = N.next_ray_rk(S, rkpos[kr], rkdir[kr], rkh[kr])
                rkpos[kr] = np_; rkdir[kr] = nd_; rkh[kr] = nh_
                cpos[kr] = np_; cdir[kr] = nd_; step[kr] = nh_
            cd = N.vlen(cpos[kr] - S.bh_pos) if N.LITERAL else N.flen(cpos[kr] - S.bh_pos)     # N7: the integrator's distance
            closest[kr] = np.where(cd < closest[kr], cd, closest[kr])
            pdir[kr] = cdir[kr]
            h_, t_, col_, op_ = N.hit_black_hole(S, ppos[kr], pdir[kr], t_min, step[kr], ray_distance[kr])
            # what hit_black_hole decided (ray.wgsl:604-611): the disk where it is hit nearer than the horizon
            hs_, ts_ = N.hit_sphere(ppos[kr], pdir[kr], f32(1.0), S.bh_pos, t_min, step[kr])
            hd_, td_ = N.hit_torus2d(ppos[kr], pdir[kr], S.inner, S.outer, S.bh_pos, S.bh_normal, t_min, step[kr])
            kind_ = np.where(hd_ & (td_ < ts_), HIT_DISK, HIT_HORIZON).astype(np.uint32)
            # ---- lensed_ref's one change: hit_ray's models behind its black hole (ray.wgsl:376-389 with render_triangles = true)
            h_ = h_.copy(); t_ = t_.copy(); col_ = col_.copy(); op_ = op_.copy()
            mi_ = np.zeros(kr.size, dtype=np.int64); tri_ = np.full(kr.size, -1, dtype=np.int64); sg_ = np.zeros(kr.size, dtype=bool)
            for j, r in enumerate(kr):
                seg = step[r]
                best_t = t_[j] if h_[j] else seg                 # closest_render_state.t: the black hole's where it hit, else t_max = the step
                won = False
                for mi in range(S.model_count):
                    m = S.models[mi]
                    if int(m.get("visible", 1)) == 0:
                        continue
                    res = RRR._trace_ray_model_slot(m, ppos[r], pdir[r], t_min, seg)   # the full range for every model
                    if res is not None and res[0] < best_t:                             # strictly nearer; a tie keeps the earlier candidate
                        tt, col, nrm, tri = res
                        diffuse = (nrm[0] * light[0] + nrm[1] * light[1]) + nrm[2] * light[2]
                        best_t = tt; won = True
                        h_[j] = True; t_[j] = tt; op_[j] = 1.0
                        col_[j] = [col[0] * diffuse, col[1] * diffuse, col[2] * diffuse]
                        kind_[j] = HIT_MESH; mi_[j] = mi; tri_[j] = tri; sg_[j] = True
                segment_hits += int(won)
            # ----
            c_hit[kr] = h_; c_t[kr] = t_; c_col[kr] = col_; c_op[kr] = op_
            c_kind[kr] = kind_; c_model[kr] = mi_; c_tri[kr] = tri_; c_seg[kr] = sg_
            out = cd > S.R
            ko = kr[out]
            if ko.size:
                rel[ko] = False
                fw = S.R * S.feather
                fs = S.R - fw
                lin = N.clamp((closest[ko] - fs) / fw, 0.0, 1.0)
                m = lin * lin
                cdir[ko] = N.mix(cdir[ko], direction[ko], m[:, None])
        if kf.size:
            h_, t_, col_, op_, mi_, tri_ = RRR._hit_models(S, cpos[kf], cdir[kf], t_min, t_max)
            hs, ts = N.hit_sphere(ppos[kf], pdir[kf], S.R, S.bh_pos, t_min, t_max)
            none = ~hs & ~h_
            alive[kf[none]] = False
            i_final[kf[none]] = it
            enter = ~none & hs & (ts < t_)
            ke = kf[enter]
            cpos[ke] = cpos[ke] + cdir[ke] * ts[enter][:, None]
            rel[ke] = True
            take = ~none & ~enter
            kt = kf[take]
            c_hit[kt] = h_[take]; c_t[kt] = t_[take]; c_col[kt] = col_[take]; c_op[kt] = op_[take]
            c_kind[kt] = HIT_MESH; c_model[kt] = mi_[take]; c_tri[kt] = tri_[take]
        ka = np.nonzero(alive & c_hit)[0]
        if ka.size:
            cpos[ka] = cpos[ka] + pdir[ka] * c_t[ka][:, None]
            cc = N.clamp(c_col[ka], 0.0, 1.0)
            color[ka] = color[ka] + cc * (amount[ka] * c_op[ka])[:, None]
            amount[ka] = amount[ka] * (f32(1.0) - c_op[ka])
            first = ka[~hit[ka]]                                   # the first accepted hit: the record's words 0-4
            if first.size:
                rec["position"][first] = cpos[first]
                mesh = c_kind[first] == HIT_MESH
                rec["hit"][first] = np.where(mesh, HIT_MESH | (c_model[first].astype(np.uint32) << 8), c_kind[first]).astype(np.uint32)
                rec["triangle"][first] = np.where(mesh, c_tri[first], -1)
                seg_first[first] = c_seg[first]
            segment_hits_after_disk += int((hit[ka] & c_seg[ka]).sum())       # a model winning a segment on a ray that had already hit (the disk): the mesh seen through it
            hit[ka] = True
        m_ = np.abs(amount - f32(0.005))
        margin = np.where(alive & (m_ < margin), m_, margin).astype(np.float32)        # the break test every live ray meets here (ray.wgsl:578)
        done = alive & (amount < f32(0.005))
        i_final[done] = it
        alive[done] = False
    out = np.zeros((n, 4), dtype=np.float32)
    colour_px = hit | (i_final <= 5)
    ks = np.nonzero(colour_px & (amount > f32(0.001)))[0]
    if ks.size:
        d = cdir[ks]
        theta = N.bh_atan2(np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]), d[:, 1])
        phi = N.bh_atan2(d[:, 2], d[:, 0])
        u = (phi + f32(2.6) * N.PI) / (f32(2.0) * N.PI)
        v = (N.PI - theta) / N.PI
        u = u - np.trunc(u); v = v - np.trunc(v)
        sc = N.sample_bilinear(S.t_sky, u, v)[:, 0:3]
        miss = (sc * sc) * (sc * sc)
        color[ks] = color[ks] + miss * amount[ks][:, None]
    out[colour_px, 0:3] = color[colour_px]; out[colour_px, 3] = 1.0
    out[~colour_px, 0:3] = cdir[~colour_px]; out[~colour_px, 3] = 0.0
    rec["position"][~hit] = cpos[~hit]
    rec["iterations"] = i_final.astype(np.uint32)
    rec["closest"] = closest
    rec["transmittance"] = amount
    return out, rec, margin, seg_first, dict(segment_hits=segment_hits, segment_hits_after_disk=segment_hits_after_disk)


# ---- the scene and the ray list --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh_dir():
    d = tempfile.mkdtemp(prefix="lensed_rays_meshes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def model(radius, pos, visible=1):
    """an 80-triangle icosphere of that radius (bhusie_amd.Model) at pos"""
    p = os.path.join(_mesh_dir(), f"ico1_{radius}.obj")
    if not os.path.exists(p):
        with open(p, "w") as f:
            f.write(assets.icosphere_mesh_obj(1, radius=float(radius)))
    m = B.load_model(p)
    m.set_transform(pos, visible)
    return m


def models(slots=None):
    return [model(*s) for s in (SLOTS if slots is None else slots)]


def uniforms(method):
    return RR.scene_uniforms(method, len(SLOTS))


@functools.lru_cache(maxsize=None)
def rays(n=N_RAYS, seed=SEED):
    """(n, 8) float32 records in thirds by index: k % 3 == 0 rays_ref.seeded_rays' construction (aimed near the hole, origins alternating inside / outside the sphere);
    k % 3 == 1 aimed at a visible mesh from inside the sphere; k % 3 == 2 aimed at one from outside"""
    rng = np.random.default_rng(seed)
    base = np.array(RR.seeded_rays(n, seed))
    vis = [s for s in SLOTS if s[2]]
    for k in range(n):
        if k % 3 == 0:
            continue
        rad, c, _ = vis[(k // 3) % len(vis)]; c = np.asarray(c, dtype=np.float64)
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        d = rng.uniform(3.0, 19.0) if k % 3 == 1 else rng.uniform(21.0, 50.0)   # inside / outside the sphere
        o = d * u
        if np.linalg.norm(o - c) < rad + 0.5:
            o = -o
        j = rng.normal(size=3); j *= rng.uniform(0.0, 1.3 * rad) / np.linalg.norm(j)
        base[k, 0:3] = o.astype(np.float32)
        base[k, 4:7] = RR._normalize32((c + j - base[k, 0:3].astype(np.float64))[None, :])[0]
    base.setflags(write=False)
    return base


def trace(method, ray_list, slots=None, trees=None):
    """trace_rays_lensed_records of (n, 8) ray records under uniforms(method); slots: SLOTS, or another list of (radius, position, visible) with as many entries;
    trees: None - the host-built trees -, or per slot a dict(nodes, bvh_lookup) to traverse instead (the device's)"""
    arrays = [m.arrays() for m in models(slots)]
    if trees is not None:
        for a, t in zip(arrays, trees):
            a["nodes"], a["bvh_lookup"] = t["nodes"], t["bvh_lookup"]
    ray_list = np.asarray(ray_list, dtype=np.float32)
    return trace_rays_lensed_records(RRR.np_scene(uniforms(method), arrays), ray_list[:, 0:3].copy(), ray_list[:, 4:7].copy())


def _frozen(t):
    for a in t[:4]:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference(method, n=N_RAYS):
    """(results, records, margin, seg_first, stats) of rays(n) under the scene: computed once per process, never modified"""
    return _frozen(trace(method, rays(n)))


@functools.lru_cache(maxsize=None)
def flat_reference(method, n=N_RAYS):
    """the flat-space trace of the same list in the same scene (ray_records_ref.trace): (results, records, margin, after_march)"""
    t = RRR.trace(uniforms(method), rays(n), [m.arrays() for m in models()])
    for a in t:
        a.setflags(write=False)
    return t


def conditions(method, n=N_RAYS):
    """the figures a list is held to, on the reference alone"""
    out, rec, margin, seg_first, st = reference(method, n)
    flat_out = flat_reference(method, n)[0]
    kind = rec["hit"] & 0xFF
    slot = (rec["hit"] >> 8) & 0xFF
    mesh = kind == HIT_MESH
    c = {"segment_hits": st["segment_hits"], "segment_hits_after_disk": st["segment_hits_after_disk"],
         "mesh_first_by_segment": int((mesh & seg_first).sum()), "mesh_first_in_flat_space": int((mesh & ~seg_first).sum()),
         "horizon": int((kind == HIT_HORIZON).sum()), "disk": int((kind == HIT_DISK).sum()), "none": int((kind == HIT_NONE).sum()),
         "margin_rays": int((margin < RRR.MARGIN_BAR).sum()), "non_finite": int((~np.isfinite(out)).any(axis=1).sum()),
         "differ_from_flat": int((out.view(np.uint32) != flat_out.view(np.uint32)).any(axis=1).sum())}
    for s in range(len(SLOTS)):
        c[f"slot{s}_by_segment"] = int((mesh & seg_first & (slot == s)).sum())
    return c


# the floors (the reference's own counts, RK / Euler, stand beside them in tests/test_lensed_rays_ref_cpu.py and tests/test_gpu_lensed_rays.py)
FLOORS = {
    N_RAYS: {"segment_hits": 150, "mesh_first_by_segment": 100, "slot0_by_segment": 30, "slot2_by_segment": 30, "slot3_by_segment": 30, "mesh_first_in_flat_space": 10,
             "segment_hits_after_disk": 40, "horizon": 50, "disk": 300, "none": 200, "differ_from_flat": 100},
    N_RAYS_CPU: {"segment_hits": 40, "mesh_first_by_segment": 30, "slot0_by_segment": 8, "slot2_by_segment": 8, "slot3_by_segment": 8,
                 "segment_hits_after_disk": 8, "horizon": 15, "disk": 60, "none": 50, "differ_from_flat": 30},
}


def assert_conditions(c, n):
    for k, floor in FLOORS[n].items():
        assert c[k] >= floor, (k, c[k], floor, c)
    assert c["slot1_by_segment"] == 0, c                         # the invisible slot: no record may name it
    assert c["non_finite"] == 0, c
    assert c["margin_rays"] <= RRR.MARGIN_SHARE * n, c
