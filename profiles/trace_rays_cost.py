"""Cost of ray batches, one MI355X.  Run by hand: `python profiles/trace_rays_cost.py [OUT.json]`; not a test.

 large    Mrays/s of the bench frame's pixel rays (the 1920x1080 frame's only level at `levels = 1`: about 2 M rays, cameras.pinhole_rays) through
          bhray_trace_rays_device - rays and results resident on the device, wall clock of enqueue + stream synchronisation, median of 9 after 3 -
          next to the same frame rendered with `levels = 1` (render + sync, one frame at a time, the same median).  Both integrators.
 small    latency of a 4 096-ray batch (the first 4 096 of those rays): the device variant (enqueue + synchronise) and the host variant
          (bhray_trace_rays: copy in, trace, copy out), median of 30 after 5.

The ray-list kernels exist in the latency build only: if `large` is far below the frame's number, that is the starting point for a dense build."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
sys.path.insert(0, ROOT)


def med_s(fn, n, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    import numpy as np
    import bhusie_amd as B
    from bhusie_amd import assets, cameras
    hip = C.CDLL("libamdhip64.so")
    tex = (assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    w, h = cfg.sizes()[-1]
    cam, bh = B.Camera(), B.BlackHole()
    rays = np.ascontiguousarray(cameras.pinhole_rays(cam, w, h))
    n = rays.shape[0]
    out = {"level": [w, h], "rays": n}
    assert hip.hipSetDevice(0) == 0
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    d_rays, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_rays), C.c_size_t(rays.nbytes)) == 0 and hip.hipMalloc(C.byref(d_out), C.c_size_t(n * 16)) == 0
    assert hip.hipMemcpy(d_rays, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), 1) == 0
    for method, name in ((1, "rk"), (0, "euler")):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex)
        rp.set_uniforms(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=method).uniform())

        def frame():
            rp.render(); rp.sync()

        def batch(count):
            rp.trace_rays_device(d_rays.value, count, d_out.value, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0

        t_frame = med_s(frame, 9, 3)
        t_large = med_s(lambda: batch(n), 9, 3)
        t_small = med_s(lambda: batch(4096), 30, 5)
        t_small_host = med_s(lambda: rp.trace_rays(rays[:4096]), 30, 5)
        rp.sync()
        out[name] = {"frame_levels1_ms": round(t_frame * 1e3, 4), "frame_levels1_mrays_s": round(w * h / t_frame / 1e6, 1),
                     "rays_device_ms": round(t_large * 1e3, 4), "rays_device_mrays_s": round(n / t_large / 1e6, 1),
                     "batch4096_device_ms": round(t_small * 1e3, 4), "batch4096_host_ms": round(t_small_host * 1e3, 4)}
        print(name, out[name], flush=True)
    hip.hipFree(d_rays); hip.hipFree(d_out); hip.hipStreamDestroy(stream)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
