"""Ray paths (bhray_trace_rays_paths) restated in NumPy: the reference the GPU tests compare with.

`trace_rays_paths` below is `tests/ray_records_ref.trace_rays_records` written out again - the same statements over np_ray's own primitives and that file's `_hit_models` -
with the bookkeeping a path needs added and nothing else changed:

  * point 0 of every ray is (origin, 0);
  * at the end of a loop pass every ray that is still alive appends (curr.position, it + 1): the shader's `i++` - curr.position as it stands then, i.e. after
    curr + prev.direction * t on a hit and after the move to the sphere's surface on an entry;
  * a ray that ends - nothing found in flat space, the transmittance below 0.005, the iteration limit - appends (curr.position, i_final): the end point, always;
  * `sample(path, s)` keeps the points whose iteration is a multiple of 2^s and the end point: what the kernels store at stride_log2 = s.

Also here: the references over rays_ref.seeded_rays()[:N_SEEDED] and ray_records_ref.mesh_rays(), computed once.
"""
from __future__ import annotations

import functools

import numpy as np

from bhusie_amd import PATH_POINT_DTYPE, RAY_RECORD_DTYPE, HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH
from oracle import np_ray as N
from tests import ray_records_ref as R
from tests import rays_ref as RR
from tests.ray_records_ref import _hit_models

f32 = np.float32
N_SEEDED = 1027                 # rays of rays_ref.seeded_rays() the path tests use: not a multiple of 64, 17 waves
MAX_POINTS = 1024               # checked in tests/test_ray_paths_ref.py: the longest of them takes 328 iterations with Euler, 811 with RK - nothing is dropped at stride 1


def trace_rays_paths(S: N.Scene, origin, direction):
    """-> ray_records_ref.trace_rays_records' four outputs - results (n, 4) float32, records (n,) RAY_RECORD_DTYPE, margin (n,) float32, after_march (n,) bool -, then
    paths: a list of n PATH_POINT_DTYPE arrays, ray r's points at stride 1 (the origin, one point per counted iteration, the end point), and counts (n,) uint32 = their lengths"""
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
    # ---- the paths' bookkeeping: row r holds ray r's points at stride 1, npts[r] of them
    pts = np.zeros((n, S.max_iter + 2), dtype=PATH_POINT_DTYPE)
    pts["position"][:, 0] = origin                  # k = 0: (origin, 0)
    npts = np.ones(n, dtype=np.int64)

    def append(rows, iteration):
        pts["position"][rows, npts[rows]] = cpos[rows]
        pts["iteration"][rows, npts[rows]] = iteration
        npts[rows] += 1

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
            append(kf[none], it)                               # the end point of a ray that finds nothing: the flat iteration did not move it
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
        append(np.nonzero(done)[0], it)                        # the end point of a ray that breaks on its transmittance
        append(np.nonzero(alive)[0], it + 1)                   # the loop's i++: a body ended and the ray goes on
    append(np.nonzero(alive)[0], S.max_iter)                   # the end point of a ray that met the iteration limit
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
    paths = [pts[r, :npts[r]].copy() for r in range(n)]
    return out, rec, margin, after_march, paths, npts.astype(np.uint32)


def sample(path, s):
    """the points of a stride-1 path that a launch with stride_log2 = s stores: iteration % 2^s == 0 among all but the last, then the end point"""
    body = path[:-1]
    keep = (body["iteration"] & np.uint32((1 << s) - 1)) == 0
    return np.concatenate([body[keep], path[-1:]])


def counts(records, s):
    return (records["iterations"] >> np.uint32(s)) + np.uint32(2)


def rows(paths, s, max_points):
    """the (n, max_points) array and the counts the host form returns for these stride-1 paths: sampled, cut at max_points, zero behind a ray's last point"""
    out = np.zeros((len(paths), max_points), dtype=PATH_POINT_DTYPE)
    cnt = np.zeros(len(paths), dtype=np.uint32)
    for r, p in enumerate(paths):
        q = sample(p, s)
        cnt[r] = q.shape[0]
        out[r, :min(q.shape[0], max_points)] = q[:max_points]
    return out, cnt


def trace(uniforms, rays, models=()):
    """trace_rays_paths of (n, 8) ray records under the uniforms' scene and tests.common's textures"""
    rays = np.asarray(rays, dtype=np.float32)
    return trace_rays_paths(R.np_scene(uniforms, models), rays[:, 0:3].copy(), rays[:, 4:7].copy())


def _frozen(t):
    for a in t:
        for b in (a if isinstance(a, list) else [a]):
            b.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def seeded_reference(method):
    """trace_rays_paths' six outputs for rays_ref.seeded_rays()[:N_SEEDED] under rays_ref.scene_uniforms(method): computed once, never modified"""
    return _frozen(trace(RR.scene_uniforms(method), RR.seeded_rays()[:N_SEEDED]))


@functools.lru_cache(maxsize=None)
def mesh_reference(method=1):
    """the same for ray_records_ref.mesh_rays() with its three model slots"""
    return _frozen(trace(R.mesh_uniforms(method), R.mesh_rays(), [m.arrays() for m in R.mesh_models()]))
