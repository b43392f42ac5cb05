#!/usr/bin/env python3
"""What does the ORDER of the phases inside one round of the trace kernel cost in lane occupancy of the step loop?  (EXPERIMENTS.md R9.1)
queue_order_sim.py's model of the persistent trace kernel (waves of 64 lanes, batches of 16 steps, a refill from the shared queue when >= 16 lanes
are empty or nobody marches) extended with the phases between the batches and a ray's way out:
  a ray marches `iterations` steps with its disk hits spaced evenly along them (a hit pauses the lane until the next shade phase);
  a ray that ESCAPES (closest approach >= 1.02 and under the iteration limit) leaves the sphere with its last step, waits for a flat iteration that sends it
  back as an "odd" lane, takes ONE general step with the wave, leaves again, waits for its second flat iteration, and then for the epilogue;
  every other ray (absorbed, opaque, out of iterations) goes from its last step to the epilogue;
  the epilogue empties the lane, and an empty lane waits for the refill.
Run over the LAST level's rays of the 1920x1080 bench frame (each ray's iterations, disk hits and closest approach from the CPU oracle's per-ray diagnostics,
the queue in the classify kernel's order) for today's order of the phases and the alternatives.  Costs: a step of the batch and the general step are one
wave-step each, the phases 0.5 wave-step per round plus 4 per shade phase that runs.  All waves take their rounds in lockstep (as queue_order_sim.py).
Prints lane-steps / (64 x wave-steps of the step loop) and the wave-steps with phase costs relative to today's order.  CPU only: python profiles/phase_order_sim.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhusie_amd as B  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import common as T  # noqa: E402

EMPTY, REL, SHADE, FLAT, FINISH = 0, 1, 2, 3, 4
PHASE_COST, SHADE_COST = 0.5, 4.0


def bench_rays():
    tex = T.textures(small=False)
    u = T.uniforms(integration_method=1)
    sc = T.oracle_scene(*u, tex)
    cfg = B.ladder_for_frame((1920, 1080), 3, 4)
    sizes = cfg.sizes()
    imgs = O.render_ladder(sc, sizes)
    kind = O.classify_level(sc, sizes[-1], imgs[-2])
    aux = O.render_aux(sc, sizes[-1])
    cx, cy = int(cfg.crop_x), int(cfg.crop_y)
    ys, xs = np.nonzero(kind[cy:cy + 1080, cx:cx + 1920] == 2)
    ys += cy; xs += cx
    tx, ty = (xs - cx) // 8, (ys - cy) // 8
    block = (ty // 2) * ((1920 // 8 + 3) // 4) + tx // 4
    order = np.lexsort((((ys - cy) % 8) * 8 + (xs - cx) % 8, (ty % 2) * 4 + tx % 4, block))          # the classify kernel's queue order
    ys, xs = ys[order], xs[order]
    length = np.maximum(aux[ys, xs, 1].astype(np.int64), 1)
    hits = aux[ys, xs, 3].astype(np.int64)
    escapes = (aux[ys, xs, 0] >= 1.02) & (length < 2000)
    return length, np.minimum(hits, length - 1), escapes


def simulate(length, hits, escapes, rotate, flat2, waves=2048, refill_min=16, batch=16, early_break=0):
    """-> (lane occupancy of the step loop, wave-steps of the step loop, wave-steps with phase costs)"""
    n = len(length); head = 0
    mode = np.zeros((waves, 64), dtype=np.int8)
    left = np.zeros((waves, 64), dtype=np.int64)       # steps to the lane's next event
    seg = np.zeros((waves, 64), dtype=np.int64)        # ... between two disk hits
    nhit = np.zeros((waves, 64), dtype=np.int64)       # disk hits still ahead
    esc = np.zeros((waves, 64), dtype=bool)
    exits = np.zeros((waves, 64), dtype=np.int8)       # 0: marching, 1: left the sphere once (the flat iteration sends it back odd), 2: left it for good
    odd = np.zeros((waves, 64), dtype=bool)
    alive = np.ones(waves, dtype=bool)
    tot = dict(lane=0, steps=0.0, cost=0.0)

    def step(which):                                   # one step of the waves `which` for their lanes in REL
        act = (mode == REL) & which[:, None]
        tot["lane"] += int(act.sum()); tot["steps"] += float(which.sum()); tot["cost"] += float(which.sum())
        left[act] -= 1
        ev = act & (left <= 0)
        hit = ev & (nhit > 0)
        mode[hit] = SHADE; nhit[hit] -= 1; left[hit] = seg[hit]
        end = ev & ~hit
        out = end & esc
        mode[out] = FLAT; exits[out] += 1; odd[out] = False
        mode[end & ~esc] = FINISH
        return ev

    def general():                                     # the wave takes ONE general step when it holds an odd lane
        w = ((mode == REL) & odd).any(axis=1) & alive
        if w.any():
            step(w)

    def march():
        general()
        gone = np.zeros(waves, dtype=np.int64)
        on = alive.copy()
        for k in range(batch):
            if k % 2 == 0:                             # (the pairs test for "nobody marches" once per pair)
                on &= (mode == REL).any(axis=1)
                if early_break:
                    on &= gone < early_break
            if not on.any():
                break
            gone += step(on).sum(axis=1)

    def shade():
        s = mode == SHADE
        tot["cost"] += SHADE_COST * float((s.any(axis=1) & alive).sum())
        mode[s] = REL

    def flat():
        f = mode == FLAT
        back = f & (exits == 1)
        mode[back] = REL; odd[back] = True; left[back] = 1; nhit[back] = 0
        mode[f & (exits >= 2)] = FINISH

    def epilogue():
        mode[mode == FINISH] = EMPTY

    def refill():
        nonlocal head
        empty = mode == EMPTY
        need = empty.sum(axis=1)
        want = alive & (need > 0) & ((need >= refill_min) | ~(mode == REL).any(axis=1))
        if head < n:
            for w in np.nonzero(want)[0]:
                k = min(need[w], n - head)
                if k <= 0:
                    break
                idx = np.nonzero(empty[w])[0][:k]
                L, Hn = length[head:head + k], hits[head:head + k]
                s = np.maximum(L // (Hn + 1), 1)
                mode[w, idx] = REL; seg[w, idx] = s; nhit[w, idx] = Hn; left[w, idx] = np.where(Hn > 0, s, L)
                esc[w, idx] = escapes[head:head + k]; exits[w, idx] = 0; odd[w, idx] = False
                head += k
        alive[:] = alive & (mode != EMPTY).any(axis=1)

    while True:
        refill()
        if not alive.any():
            break
        tot["cost"] += PHASE_COST * float(alive.sum())
        if rotate:
            march()
        shade()
        flat()
        if flat2:
            general(); flat()
        epilogue()
        if not rotate:
            march()
    return tot["lane"] / (64.0 * tot["steps"]), tot["steps"], tot["cost"]


if __name__ == "__main__":
    length, hits, escapes = bench_rays()
    print("rays %d, mean iterations %.1f, escaping %.1f %%, disk hits per ray %.2f" % (len(length), length.mean(), 100.0 * escapes.mean(), hits.mean()))
    base = None
    for name, kw in (("today's order: refill, shade, flat, epilogue, march", dict(rotate=False, flat2=False)),
                     ("refill behind the epilogue, in front of the march", dict(rotate=True, flat2=False)),
                     ("flat phase repeated behind the general step", dict(rotate=False, flat2=True)),
                     ("both", dict(rotate=True, flat2=True)),
                     ("both + 8-step batches", dict(rotate=True, flat2=True, batch=8)),
                     ("both + batch broken when 16 lanes have left", dict(rotate=True, flat2=True, early_break=16)),
                     ("both + batch broken when 8 lanes have left", dict(rotate=True, flat2=True, early_break=8)),
                     ("today's order + 8-step batches", dict(rotate=False, flat2=False, batch=8))):
        occ, steps, cost = simulate(length, hits, escapes, **kw)
        if base is None:
            base = (steps, cost)
        print("%-58s lane occupancy %.4f   wave-steps %.4f   with phase costs %.4f" % (name, occ, steps / base[0], cost / base[1]))
