"""Cost of lensed meshes (bhray_set_mesh_lensing), one MI355X.

`python profiles/lensed_cost.py [OUT.json] [--off-only] [--rounds N]`: ms per frame at 1920x1080, adaptive RK, the mesh of
bench.py --workload mesh (327 680 triangles), in 20-frame blocks (22 frame slots, 2 speculative levels; median of 5 blocks after 2) and
one frame at a time (median of 12 after 3), for

 off          lensing off (the kernels every frame used before the mode existed), mesh where bench.py puts it: (-10, 0, 30), outside R = 20
 on_outside   lensing on, the same scene: no segment inside the sphere reaches the mesh, so only the per-step cull is paid
 on_inside    lensing on, the mesh moved to (4, 0, -8): in front of the default camera, inside the sphere

--off-only measures the first leg alone, N rounds: with BHRAY_LIB pointing at a library built from the parent tree (and BHRAY_AB_OLD_BUILD=1,
which lets the bindings skip the symbol that library lacks) it is the other side of an alternating A/B of that leg."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts


def med_ms(fn, n, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 4)


def leg(B, cfg, tex, model, position, lensed):
    out = {}
    for name, kw in (("block20", dict(frames_in_flight=22, speculative_levels=2)), ("one_frame", dict(frames_in_flight=1, speculative_levels=2))):
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        rp.upload_model(model)
        rp.set_model_transform(position, 1)
        if lensed:
            rp.set_mesh_lensing(1)
        det = B.RayDetails(integration_method=1, model_count=1)
        cam, bh = B.Camera(), B.BlackHole()
        k = [0]

        def frame():
            det.time = k[0] / 60.0; k[0] += 1
            rp.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())
            rp.render()

        def block():
            for _ in range(20):
                frame()
            rp.sync()

        def one():
            frame(); rp.sync()
        if name == "block20":
            out["block20_ms_per_frame"] = round(med_ms(block, 5, 2) / 20.0, 4)
        else:
            out["one_frame_ms"] = med_ms(one, 12, 3)
        rp.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    import bhusie_amd as B
    from bhusie_amd import assets
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    off_only = "--off-only" in sys.argv
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 1
    if "--rounds" in sys.argv:
        args = [a for a in args if a != sys.argv[sys.argv.index("--rounds") + 1]]
    tex = (assets.temp_lut(256), assets.reference_disk_texture(1000), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 4)
    with tempfile.NamedTemporaryFile("w", suffix=".obj", delete=False) as f:
        f.write(assets.icosphere_mesh_obj(7, radius=8.0, bump=0.15, seed=3))
        path = f.name
    model = B.load_model(path)
    os.unlink(path)
    outside, inside = (-10.0, 0.0, 30.0), (4.0, 0.0, -8.0)
    res = {"source": "profiles/lensed_cost.py, one MI355X; wall clock, ms per frame", "frame": [int(cfg.frame_w), int(cfg.frame_h)],
           "library": os.path.basename(B.LIB_PATH), "triangles": int(len(model.arrays()["triangles"]))}
    res["off"] = [leg(B, cfg, tex, model, outside, False) for _ in range(rounds)]
    print("off", res["off"], flush=True)
    if not off_only:
        res["on_outside"] = leg(B, cfg, tex, model, outside, True)
        print("on_outside", res["on_outside"], flush=True)
        res["on_inside"] = leg(B, cfg, tex, model, inside, True)
        print("on_inside", res["on_inside"], flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
