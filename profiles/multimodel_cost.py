"""Cost of several models per ctx, wall clock on one MI355X.

`python profiles/multimodel_cost.py [OUT.json]` renders the configs[2] scene of bench.py --workload mesh (1920x1080, 72x41 x3 x4 ladder,
adaptive RK, the 327 680-triangle icosphere) with N = 1, 2, 4 and 8 copies of its mesh in slots 0 .. N-1, placed on the circle of the
default model position (-10, 0, 30) around the hole (N = 1 is exactly bench.py's scene), and N = 8 with copy 0 there and seven copies
behind the camera.  Two figures per scene, as bench.py measures them: ms per frame of a 20-frame block (22 frame slots, 2 speculative
levels, time += 1/60 per frame; median of 5 blocks after 2 warm-up blocks) and ms for one frame rendered and synchronised alone (one
frame slot, 2 speculative levels; median of 12 after 3).  Prints the JSON summary and writes it to OUT.json when given
(profiles/r08_multimodel_cost.json)."""
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts: 22 frame slots on fewer queues would serialise


def placements(n, behind=False):
    base = (-10.0, 0.0, 30.0)
    if behind:                                                  # copies 1-7 far behind the camera (0, 0, -19), 24 units apart
        return [base] + [(-72.0 + 24.0 * k, 0.0, -150.0) for k in range(7)]
    r, a0 = math.hypot(base[0], base[2]), math.atan2(base[2], base[0])
    return [(r * math.cos(a0 + 2.0 * math.pi * k / n), 0.0, r * math.sin(a0 + 2.0 * math.pi * k / n)) for k in range(n)]


def measure(B, cfg, tex, model, poses):
    out = {}
    for name, kw in (("block20", dict(frames_in_flight=22, speculative_levels=2)), ("one_frame", dict(frames_in_flight=1, speculative_levels=2))):
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        for i, p in enumerate(poses):
            model.set_transform(p, 1)
            rp.upload_model(model, i)
        det = B.RayDetails(integration_method=1, model_count=len(poses))
        cam, bh = B.Camera(), B.BlackHole()
        k = 0

        def frame():
            nonlocal k
            det.time = k / 60.0; k += 1
            rp.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())
            rp.render()
        if name == "block20":
            ts = []
            for b in range(7):
                t0 = time.perf_counter()
                for _ in range(20):
                    frame()
                rp.sync()
                ts.append((time.perf_counter() - t0) / 20.0)
            out["block20_ms_per_frame"] = round(statistics.median(ts[2:]) * 1e3, 4)
        else:
            for _ in range(3):
                frame(); rp.sync()
            ts = []
            for _ in range(12):
                t0 = time.perf_counter()
                frame(); rp.sync()
                ts.append(time.perf_counter() - t0)
            out["one_frame_ms"] = round(statistics.median(ts) * 1e3, 4)
        rp.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    import bhusie_amd as B
    from bhusie_amd import assets
    tex = (assets.temp_lut(256), assets.reference_disk_texture(1000), assets.sky_texture(4096, 2048, seed=2))
    with tempfile.NamedTemporaryFile("w", suffix=".obj", delete=False) as f:
        f.write(assets.icosphere_mesh_obj(7, radius=8.0, bump=0.15, seed=3))          # bench.py --workload mesh
        path = f.name
    model = B.load_model(path)
    os.unlink(path)
    cfg = B.ladder_from_base((72, 41), 3, 4)
    res = {"source": "profiles/multimodel_cost.py, wall clock, one MI355X; configs[2] (1918x1081 ladder, adaptive RK, 327 680 triangles per copy)",
           "frame": list(cfg.sizes()[-1])}
    for n in (1, 2, 4, 8):
        res[f"N{n}_around_the_hole"] = dict(measure(B, cfg, tex, model, placements(n)), positions=[list(p) for p in placements(n)])
        print(n, res[f"N{n}_around_the_hole"], flush=True)
    res["N8_seven_behind_the_camera"] = dict(measure(B, cfg, tex, model, placements(8, behind=True)), positions=[list(p) for p in placements(8, True)])
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
