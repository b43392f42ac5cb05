"""Ray records (bhray_trace_rays_records) restated in NumPy: the reference the GPU tests compare with.

`trace_rays_records` below is `oracle.np_ray.trace_rays` written out again - the same statements over np_ray's own primitives (next_ray_*, hit_black_hole, hit_sphere,
_hit_aabb, _hit_triangle) - with the bookkeeping a record needs added and nothing else changed:

  * where the shader sets `hit = true` for the FIRST time (ray.wgsl:570) the ray's record takes curr.position (just moved by prev.direction * t, ray.wgsl:571), what was
    hit - the horizon or the disk (hit_black_hole's own decision, taken again from hit_sphere / hit_torus2d), or a mesh - and for a mesh the model's index and the triangle;
  * the traversal is np_ray.trace_ray_model's text with one addition: it remembers `bvh_lookup[contents + i]` of the triangle that won (an index into the model's
    `triangles` as the caller holds them), and the models' loop remembers which model's hit stands;
  * when the loop ends: i, closest_to_bh and color_amount; a ray that never hit records curr.position there;
  * `margin`: the smallest |color_amount - 0.005| the loop's break test (ray.wgsl:578) saw.  The disk's opacity is held to 1e-4, not to bits, so a ray whose margin is
    below that may legitimately break one iteration earlier or later on another implementation: the comparisons leave such rays out.

Also here: the ray list of the mesh test (`mesh_rays`, two copies of rays_ref.mesh_model() in slots 0 and 2, slot 1 invisible) and the references, computed once.
"""
from __future__ import annotations

import functools

import numpy as np

import bhusie_amd as B
from bhusie_amd import RAY_RECORD_DTYPE, HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH
from oracle import np_ray as N
from tests import common as T
from tests import rays_ref as RR

f32 = np.float32
MARGIN_BAR = 1e-4               # rays whose break test came this close to 0.005 are left out of the exact comparisons ...
MARGIN_SHARE = 0.01             # ... and may be at most this share of a list


def _trace_ray_model_slot(m, pos, dirn, t_min, t_max):
    """np_ray.trace_ray_model, returning (t, colour, normal, triangle) of the nearest hit: triangle = bvh_lookup[contents + i] of the leaf slot that won"""
    nodes, lookup, tris, pts, nrm = m["nodes"], m["bvh_lookup"], m["triangles"], m["points"], m["normals"]
    off = N._s3(m["position"])
    pos = N._s3(pos); dirn = N._s3(dirn)
    best = None; best_t = f32(t_max)
    node = 0; stack = []
    while True:
        nd = nodes[node]
        cnt, contents = int(nd["obj_count"]), int(nd["left_child"])
        if cnt == 0:
            c1, c2 = contents, contents + 1
            d1 = N._hit_aabb(pos, dirn, nodes[c1], off); d2 = N._hit_aabb(pos, dirn, nodes[c2], off)
            if d1 > d2:
                d1, d2, c1, c2 = d2, d1, c2, c1
            if d1 > best_t:
                if not stack:
                    break
                node = stack.pop()
            else:
                node = c1
                if d2 < best_t:
                    stack.append(c2)
        else:
            for i in range(cnt):
                tri = int(lookup[contents + i])
                ti = tris[tri]
                P = [tuple(f32(pts[int(ti[k])][a]) + off[a] for a in range(3)) for k in range(3)]
                Nn = [N._s3(nrm[int(ti[3 + k])]) for k in range(3)]
                r = N._hit_triangle(pos, dirn, f32(t_min), f32(t_max), P[0], P[1], P[2], Nn[0], Nn[1], Nn[2])
                if r is not None and r[0] < best_t:
                    best, best_t = r + (tri,), r[0]
            if not stack:
                break
            node = stack.pop()
    return best


def _hit_models(S: N.Scene, pos, dirn, t_min, t_max):
    """np_ray.hit_models, returning also the model index and the triangle of the hit that stands (-1 where none)"""
    n = pos.shape[0]
    hit = np.zeros(n, dtype=bool); t = np.full(n, f32(t_max), dtype=np.float32)
    color = np.zeros((n, 3), dtype=np.float32); opacity = np.zeros(n, dtype=np.float32)
    model = np.full(n, -1, dtype=np.int64); triangle = np.full(n, -1, dtype=np.int64)
    if S.model_count <= 0:
        return hit, t, color, opacity, model, triangle
    l0 = (f32(0.2), f32(0.2), f32(-1.0))
    ll = np.sqrt((l0[0] * l0[0] + l0[1] * l0[1]) + l0[2] * l0[2]); lr = f32(1.0) / ll
    light = (l0[0] * lr, l0[1] * lr, l0[2] * lr)
    for r in range(n):
        for mi in range(S.model_count):
            m = S.models[mi]
            if int(m.get("visible", 1)) == 0:
                continue
            res = _trace_ray_model_slot(m, pos[r], dirn[r], t_min, t_max)
            if res is not None and res[0] < t[r]:
                tt, col, nrm, tri = res
                diffuse = (nrm[0] * light[0] + nrm[1] * light[1]) + nrm[2] * light[2]
                hit[r] = True; t[r] = tt; opacity[r] = 1.0
                color[r] = [col[0] * diffuse, col[1] * diffuse, col[2] * diffuse]
                model[r] = mi; triangle[r] = tri
    return hit, t, color, opacity, model, triangle


def trace_rays_records(S: N.Scene, origin, direction):
    """-> (results (n, 4) float32 - np_ray.trace_rays' -, records (n,) RAY_RECORD_DTYPE, margin (n,) float32, flat_first (n,) bool: the first hit came in a flat-space
    iteration AFTER the ray had marched through the sphere)"""
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
    marched = np.zeros(n, dtype=bool)              # the ray has taken an integrator step
    after_march = np.zeros(n, dtype=bool)
    for it in range(S.max_iter):
        if not alive.any():
            break
        c_hit = np.zeros(n, dtype=bool); c_t = np.zeros(n, dtype=np.float32)
        c_col = np.zeros((n, 3), dtype=np.float32); c_op = np.zeros(n, dtype=np.float32)
        c_kind = np.zeros(n, dtype=np.uint32); c_model = np.zeros(n, dtype=np.int64); c_tri = np.full(n, -1, dtype=np.int64)
        kr = np.nonzero(alive & rel)[0]
        kf = np.nonzero(alive & ~rel)[0]
        if kr.size:
            marched[kr] = True
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
            c_hit[kr] = h_; c_t[kr] = t_; c_col[kr] = col_; c_op[kr] = op_
            # what hit_black_hole decided (ray.wgsl:604-611): the disk where it is hit nearer than the horizon
            hs_, ts_ = N.hit_sphere(ppos[kr], pdir[kr], f32(1.0), S.bh_pos, t_min, step[kr])
            hd_, td_ = N.hit_torus2d(ppos[kr], pdir[kr], S.inner, S.outer, S.bh_pos, S.bh_normal, t_min, step[kr])
            c_kind[kr] = np.where(hd_ & (td_ < ts_), HIT_DISK, HIT_HORIZON)
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
            h_, t_, col_, op_, mi_, tri_ = _hit_models(S, cpos[kf], cdir[kf], t_min, t_max)
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
                after_march[first] = marched[first] & mesh
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
    return out, rec, margin, after_march


def np_scene(uniforms, models=()):
    cam, bh, det = uniforms
    tex = T.textures()
    return N.Scene(cam, bh, det, tex[0], tex[1], tex[2], list(models))


def trace(uniforms, rays, models=()):
    """trace_rays_records of (n, 8) ray records under the uniforms' scene and tests.common's textures"""
    rays = np.asarray(rays, dtype=np.float32)
    return trace_rays_records(np_scene(uniforms, models), rays[:, 0:3].copy(), rays[:, 4:7].copy())


def _frozen(t):
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def seeded_reference(method):
    """(results, records, margin, after_march) of rays_ref.seeded_rays() under rays_ref.scene_uniforms(method): computed once, never modified"""
    return _frozen(trace(RR.scene_uniforms(method), RR.seeded_rays()))


# ---- the mesh test's own list ----------------------------------------------------------------------------------------------------
N_MESH_RAYS = 1003              # not a multiple of 64
MESH_SEED = 20240713
MESH_SLOTS = {0: (-18.0, 6.0, 30.0), 1: (0.0, 40.0, 0.0), 2: (26.0, -8.0, 22.0)}     # slot 1 is uploaded invisible: no record may name it
MESH_VISIBLE = {0: 1, 1: 0, 2: 1}


def mesh_models():
    """three copies of rays_ref.mesh_model() (bhusie_amd.Model), slot by slot"""
    ms = []
    for slot in (0, 1, 2):
        m = RR.mesh_model(MESH_SLOTS[slot])
        m.set_transform(MESH_SLOTS[slot], MESH_VISIBLE[slot])
        ms.append(m)
    return ms


@functools.lru_cache(maxsize=None)
def mesh_rays(n=N_MESH_RAYS, seed=MESH_SEED):
    """(n, 8) float32 records aimed at the two visible meshes, alternating between them.  Even pairs start beyond the mesh, outside the relativity sphere, and look back
    at it: the mesh is their first flat-space iteration.  Odd pairs start on the FAR side of the hole, inside the sphere, pass the hole well outside the disk and leave the
    sphere towards the mesh: they march before the flat-space hit."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 8), dtype=np.float32)
    for k in range(n):
        c = np.asarray(MESH_SLOTS[0 if (k % 2) == 0 else 2], dtype=np.float64)
        u = c / np.linalg.norm(c)
        w = np.cross(u, [0.0, 1.0, 0.0]); w /= np.linalg.norm(w)
        v = np.cross(u, w)
        jitter = rng.normal(size=3); jitter *= rng.uniform(0.0, 7.0) / np.linalg.norm(jitter)
        if ((k // 2) % 2) == 0:
            origin = c + u * rng.uniform(18.0, 30.0) + 6.0 * (rng.uniform(-1, 1) * w + rng.uniform(-1, 1) * v)
            target = c + jitter
        else:
            side = v if v[1] > 0 else -v                       # pass above the disk's plane, which lies near y = 0
            origin = -u * rng.uniform(10.0, 17.0) + side * rng.uniform(11.0, 15.0) + w * rng.uniform(-3.0, 3.0)
            target = c + side * rng.uniform(8.0, 16.0) + jitter
        rec[k, 0:3] = origin.astype(np.float32)
        rec[k, 4:7] = RR._normalize32((target - rec[k, 0:3].astype(np.float64))[None, :])[0]
    rec.setflags(write=False)
    return rec


def mesh_uniforms(method):
    return RR.scene_uniforms(method, 3)


def mesh_trace(method, trees=None):
    """the restatement over mesh_rays(); trees: None - the host-built trees of mesh_models() -, or per slot a dict(nodes, bvh_lookup) to traverse instead (the device's)"""
    arrays = [m.arrays() for m in mesh_models()]
    if trees is not None:
        for a, t in zip(arrays, trees):
            a["nodes"], a["bvh_lookup"] = t["nodes"], t["bvh_lookup"]
    return _frozen(trace(mesh_uniforms(method), mesh_rays(), arrays))


@functools.lru_cache(maxsize=None)
def mesh_reference(method=1):
    return mesh_trace(method)


def mesh_conditions(rec, after_march):
    """the figures the mesh list is held to, on the reference alone"""
    kind = rec["hit"] & 0xFF
    slot = (rec["hit"] >> 8) & 0xFF
    mesh = kind == HIT_MESH
    return {"mesh_slot0": int((mesh & (slot == 0)).sum()), "mesh_slot2": int((mesh & (slot == 2)).sum()), "mesh_slot1": int((mesh & (slot == 1)).sum()),
            "after_march": int((mesh & after_march).sum()), "triangles": int(len(set(zip(slot[mesh].tolist(), rec["triangle"][mesh].tolist())))),
            "distinct_triangle_indices": int(len(np.unique(rec["triangle"][mesh])))}


def kinds(rec):
    k = rec["hit"] & 0xFF
    return {"none": int((k == HIT_NONE).sum()), "horizon": int((k == HIT_HORIZON).sum()), "disk": int((k == HIT_DISK).sum()), "mesh": int((k == HIT_MESH).sum())}
