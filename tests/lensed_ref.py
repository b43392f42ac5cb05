"""Lensed meshes (bhray_set_mesh_lensing) restated in NumPy: the reference the GPU tests compare with.

The mode is the shader's relativity iteration with one literal changed: ray.wgsl:541 becomes
`hit_ray(prev_ray, t_min, step_size, ray_distance, true, true)`.  `trace_rays_lensed` below is `oracle.np_ray.trace_rays` written out
again with that one change: behind `hit_black_hole` of the relativity branch a per-ray loop runs the models of `hit_ray`
(ray.wgsl:376-389) over the segment - the previous position with the NEW direction, range (t_min, step) - every model with the full
range, a strictly nearer hit replacing what stands (the black hole's result first, then the earlier models'), its colour times the
diffuse factor, opacity 1.  Everything else is np_ray's text, and everything it calls is np_ray's own.

`render_ladder_lensed` swaps the function into `np_ray.render_level` for the call; `stats` also counts "segment_hits", the segments on
which a model won.
"""
from __future__ import annotations

import numpy as np

from oracle import np_ray as N

f32 = np.float32


def _light():
    l0 = (f32(0.2), f32(0.2), f32(-1.0))
    ll = np.sqrt((l0[0] * l0[0] + l0[1] * l0[1]) + l0[2] * l0[2]); lr = f32(1.0) / ll
    return (l0[0] * lr, l0[1] * lr, l0[2] * lr)


def trace_rays_lensed(S: N.Scene, origin, direction, stats=None):
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
    steps = 0
    segment_hits = 0
    light = _light()
    for it in range(S.max_iter):
        if not alive.any():
            break
        c_hit = np.zeros(n, dtype=bool); c_t = np.zeros(n, dtype=np.float32)
        c_col = np.zeros((n, 3), dtype=np.float32); c_op = np.zeros(n, dtype=np.float32)
        kr = np.nonzero(alive & rel)[0]
        kf = np.nonzero(alive & ~rel)[0]
        if kr.size:
            steps += kr.size
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
            # ---- the one change: hit_ray's models behind its black hole (ray.wgsl:376-389 with render_triangles = true)
            if S.model_count > 0:
                h_ = h_.copy(); t_ = t_.copy(); col_ = col_.copy(); op_ = op_.copy()
                for j, r in enumerate(kr):
                    seg = step[r]
                    best_t = t_[j] if h_[j] else seg                 # closest_render_state.t: the black hole's where it hit, else t_max = the step
                    won = False
                    for mi in range(S.model_count):
                        m = S.models[mi]
                        if int(m.get("visible", 1)) == 0:
                            continue
                        res = N.trace_ray_model(m, ppos[r], pdir[r], t_min, seg)        # the full range for every model
                        if res is not None and res[0] < best_t:                           # strictly nearer; a tie keeps the earlier candidate
                            tt, col, nrm = res
                            diffuse = (nrm[0] * light[0] + nrm[1] * light[1]) + nrm[2] * light[2]
                            best_t = tt; won = True
                            h_[j] = True; t_[j] = tt; op_[j] = 1.0
                            col_[j] = [col[0] * diffuse, col[1] * diffuse, col[2] * diffuse]
                    segment_hits += int(won)
            # ----
            c_hit[kr] = h_; c_t[kr] = t_; c_col[kr] = col_; c_op[kr] = op_
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
            h_, t_, col_, op_ = N.hit_models(S, cpos[kf], cdir[kf], t_min, t_max)
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
        ka = np.nonzero(alive & c_hit)[0]
        if ka.size:
            cpos[ka] = cpos[ka] + pdir[ka] * c_t[ka][:, None]
            cc = N.clamp(c_col[ka], 0.0, 1.0)
            color[ka] = color[ka] + cc * (amount[ka] * c_op[ka])[:, None]
            amount[ka] = amount[ka] * (f32(1.0) - c_op[ka])
            hit[ka] = True
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
    if stats is not None:
        stats["steps"] = stats.get("steps", 0) + int(steps); stats["traced"] = stats.get("traced", 0) + n
        stats["sky_samples"] = stats.get("sky_samples", 0) + int(ks.size)
        stats["segment_hits"] = stats.get("segment_hits", 0) + int(segment_hits)
    return out


def render_ladder_lensed(S: N.Scene, sizes, stats=None):
    """np_ray.render_ladder with trace_rays_lensed in trace_rays' place for the call; stats: steps, traced, sky_samples, copied,
    interpolated (np_ray's) and segment_hits."""
    plain = N.trace_rays
    N.trace_rays = trace_rays_lensed
    try:
        return N.render_ladder(S, sizes, stats)
    finally:
        N.trace_rays = plain
