#!/usr/bin/env python3
"""Evidence behind the latency work of round 2 (run on the GPU box from the repo root; writes gpurun_out/latency_experiments.json,
copied to profiles/r02_latency_experiments.json).

temporal_prediction  BHRAY_F_TEMPORAL with a moving camera: rays the per-level fix-up launches had to trace (= what the prediction
                     missed) and the latency of one frame at a time, for the prediction parameters BHRAY_TEMPORAL_MARGIN /
                     BHRAY_TEMPORAL_RADIUS="last[,below]" (the library's defaults are 0.8 and 1,4).

The recorded file also holds lone_wave_phases / lone_wave_phases_fine: where one wave's time goes in a latency-bound launch (level 0
of the 1080p ladder alone, 2 993 rays dealt out 3 per wave), per-phase and per-iteration clocks written by a timing-only build of
round 2 (-DBHRAY_EXP_PROFILE; clock64 ticks = shader clocks, 0.42 ns on the box: profiles/ubench/lone_wave.hip; every clock read
costs ~70).  That build option and its read-back export are gone, and so is the part of this script that used them.
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "gpurun_out", "latency_experiments.json")


def temporal():
    import bhusie_amd as B
    from bhusie_amd import assets
    tex = (assets.temp_lut(256), assets.reference_disk_texture(1000), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 4)
    bh, det = B.BlackHole(), B.RayDetails(integration_method=1)

    def path(n, da, dy):
        out = []
        for i in range(n):
            a = da * i
            pos = (19.0 * math.sin(a), dy * i, -19.0 * math.cos(a))
            nn = math.sqrt(sum(v * v for v in pos))
            out.append((B.Camera(position=pos, forward=tuple(-v / nn for v in pos)).uniform(), bh.uniform(), det.uniform()))
        return out
    rows = []
    for name, da, dy in (("static", 0.0, 0.0), ("orbit 0.002 rad + 0.03 up per frame", 0.002, 0.03), ("orbit 0.02 rad + 0.3 up per frame (bench.py's moving camera)", 0.02, 0.3)):
        P = path(16, da, dy)
        for margin, radius in ((1.0, "0"), (0.9, "1,4"), (0.8, "0,4"), (0.8, "1,4"), (0.8, "2,4"), (0.7, "1,2"), (0.7, "1,4"), (0.5, "2,4")):
            os.environ["BHRAY_TEMPORAL_MARGIN"] = str(margin); os.environ["BHRAY_TEMPORAL_RADIUS"] = radius
            row = {"camera": name, "margin": margin, "radius_last_below": radius}
            rp = B.RayPass(cfg, frames_in_flight=1, temporal=True)
            rp.set_textures(*tex)
            ts = []
            for i, u in enumerate(P):
                rp.set_uniforms(*u)
                t0 = time.perf_counter(); rp.render(); rp.sync()
                if i >= 3:
                    ts.append(time.perf_counter() - t0)
            rp.close()
            row["latency_ms_median"] = round(sorted(ts)[len(ts) // 2] * 1e3, 4)
            rp = B.RayPass(cfg, frames_in_flight=1, temporal=True, counters=True)
            rp.set_textures(*tex)
            fix, traced = [], []
            for i, u in enumerate(P[:9]):
                rp.set_uniforms(*u); rp.render(); rp.sync()
                if i >= 5:
                    lc = [rp.level_counters(l)["traced"] for l in range(4)]
                    fix.append(lc[1:]); traced.append(sum(lc))
            rp.close()
            row["fixup_rays_levels_1_2_3_per_frame"] = fix
            row["traced_rays_per_frame"] = traced
            rows.append(row)
            print(row, flush=True)
    return rows


if __name__ == "__main__":
    res = {"temporal_prediction": temporal()}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print("wrote", OUT)
