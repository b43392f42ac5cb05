"""Cost of building mesh BVHs on the GPU, one MI355X.

`python profiles/device_bvh_cost.py [OUT.json]` (profiles/r09_device_bvh_cost.json), for the icosphere meshes of 20 480 / 81 920 /
327 680 triangles (levels 5, 6, 7; the last is the mesh of bench.py --workload mesh):

 build    upload_ms / build_ms of bhray_get_model_build_info and the wall clock of bhray_upload_model_build and of
          bhray_update_model_vertices, median of 20 after 3 warm-up calls, against the host path timed in the same run:
          bhray_model_build_bvh + bhray_upload_model, and bhray_model_build_bvh_sah + bhray_upload_model (median of 3: they take seconds).
 trace    ms per frame of configs[2] (1918x1081 ladder, adaptive RK) in a 20-frame block (22 frame slots, 2 speculative levels; median
          of 5 blocks after 2) and one frame at a time (median of 12 after 3) with the reference tree, the SAH tree and the device tree.
 animate  frames per second of the loop update vertices -> render -> resolve_sky -> sync at 1918x1081, device path against the same loop
          through the host builder (model rebuilt with bhray_model_build_bvh and uploaded again every frame).
 pose     the same for a mesh posed on the device: wall clock of bhray_set_model_pose with its upload_ms (the pose kernel) and
          build_ms, median of 20 after 3, and frames per second of the loop set pose -> render -> resolve_sky -> sync, beside the host-update loop."""
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


def trace_cost(B, cfg, tex, upload):
    out = {}
    for name, kw in (("block20", dict(frames_in_flight=22, speculative_levels=2)), ("one_frame", dict(frames_in_flight=1, speculative_levels=2))):
        rp = B.RayPass(cfg, device=0, **kw)
        rp.set_textures(*tex)
        upload(rp)
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
    import numpy as np
    import bhusie_amd as B
    from bhusie_amd import assets
    tex = (assets.temp_lut(256), assets.reference_disk_texture(1000), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_from_base((72, 41), 3, 4)
    res = {"source": "profiles/device_bvh_cost.py, one MI355X; wall clock in ms unless named otherwise", "frame": list(cfg.sizes()[-1]), "meshes": {}}
    for level in (5, 6, 7):
        with tempfile.NamedTemporaryFile("w", suffix=".obj", delete=False) as f:
            f.write(assets.icosphere_mesh_obj(level, radius=8.0, bump=0.15, seed=3))
            path = f.name
        model = B.load_model(path)
        os.unlink(path)
        a = model.arrays()
        T = len(a["triangles"])
        moved = a["points"].copy()
        moved[:, :3] *= np.float32(1.01)
        r = {"triangles": T}
        rp = B.RayPass(cfg, device=0, frames_in_flight=1, speculative_levels=2)
        rp.set_textures(*tex)
        # -- build
        r["upload_model_build_ms"] = med_ms(lambda: rp.upload_model_build(model), 20, 3)
        flip = [0]

        def update():
            flip[0] ^= 1
            rp.update_model_vertices(moved if flip[0] else a["points"], a["normals"])
        ev = {"upload_ms": [], "build_ms": []}

        def update_and_note():
            update()
            i = rp.model_build_info()
            ev["upload_ms"].append(i["upload_ms"]); ev["build_ms"].append(i["build_ms"])
        r["update_model_vertices_ms"] = med_ms(update_and_note, 20, 3)
        r["event_upload_ms"] = round(statistics.median(ev["upload_ms"][3:]), 4)
        r["event_build_ms"] = round(statistics.median(ev["build_ms"][3:]), 4)
        info = rp.model_build_info()
        r["device_tree"] = {k: info[k] for k in ("nodes", "leaves", "max_leaf", "max_depth")}

        def host_reference():
            model.build_bvh(); rp.upload_model(model)

        def host_sah():
            model.build_bvh_sah(); rp.upload_model(model)
        r["host_build_bvh_plus_upload_ms"] = med_ms(host_reference, 3, 1)
        r["host_build_bvh_sah_plus_upload_ms"] = med_ms(host_sah, 3, 1)
        r["host_over_device_update"] = round(r["host_build_bvh_plus_upload_ms"] / r["update_model_vertices_ms"], 1)
        r["host_over_device_upload"] = round(r["host_build_bvh_plus_upload_ms"] / r["upload_model_build_ms"], 1)
        # -- animation at the frame size of configs[2]
        det = B.RayDetails(integration_method=1, model_count=1)
        cam, bh = B.Camera(), B.BlackHole()
        rp.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())

        def show():
            rp.render(); rp.resolve_sky(); rp.sync()

        def animate_device():
            update(); show()

        def animate_host():
            flip[0] ^= 1
            model.build_bvh(); rp.upload_model(model); show()
        rp.upload_model_build(model)
        r["animation_fps_device"] = round(1e3 / med_ms(animate_device, 20, 3), 2)
        r["animation_fps_host"] = round(1e3 / med_ms(animate_host, 3, 1), 3)
        # -- the posed animation: 48 bytes per frame instead of the moved arrays
        rp.upload_model_build(model)
        turn = [0]
        pv = {"upload_ms": [], "build_ms": []}

        def pose():
            turn[0] += 1
            rp.set_model_pose(B.pose_from_euler((0.0, 0.01 * turn[0], 0.0)))

        def pose_and_note():
            pose()
            i = rp.model_build_info()
            pv["upload_ms"].append(i["upload_ms"]); pv["build_ms"].append(i["build_ms"])

        def animate_pose():
            pose(); show()
        r["set_model_pose_ms"] = med_ms(pose_and_note, 20, 3)
        r["pose_event_upload_ms"] = round(statistics.median(pv["upload_ms"][3:]), 4)
        r["pose_event_build_ms"] = round(statistics.median(pv["build_ms"][3:]), 4)
        r["animation_fps_pose"] = round(1e3 / med_ms(animate_pose, 20, 3), 2)
        rp.close()
        # -- what the tree costs to trace
        model.build_bvh()
        r["trace_reference_tree"] = trace_cost(B, cfg, tex, lambda p: p.upload_model(model))
        model.build_bvh_sah()
        r["trace_sah_tree"] = trace_cost(B, cfg, tex, lambda p: p.upload_model(model))
        model.build_bvh()
        r["trace_device_tree"] = trace_cost(B, cfg, tex, lambda p: p.upload_model_build(model))
        res["meshes"][f"icosphere_{level}"] = r
        print(level, r, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
