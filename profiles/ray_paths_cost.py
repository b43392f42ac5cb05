"""Cost of ray paths, one MI355X.  Run by hand: `python profiles/ray_paths_cost.py [OUT.json]`; not a test.

What a path costs is the difference between two kernels over the same rays, results, records and points resident on the device:

 records    bhray_trace_rays_records_device: the four record kernels of DESIGN.md section 16 - the parent commit's kernels, text and resources: the yardstick.
 paths      bhray_trace_rays_paths_device at stride_log2 = 0, 3 and 6, rows sized so that nothing is dropped ((max_iterations >> s) + 2 points): the four path kernels.
            They march with the general step text where the record kernels march unified, so the difference holds both the stores and the other march.

4 096 rays of the bench frame (every 506th pixel ray of the 1920x1080 frame's only level at `levels = 1`: an even sample, cameras.pinhole_rays), wall clock of enqueue +
stream synchronisation, median of 30 after 5, the legs run in turn (A B C D A B C D ...) so that clock drift lands on all of them.  Both integrators.  ms per batch.

At s = 0 every marching lane stores 16 bytes per step, the 64 lanes of a wave to 64 different rows; at s = 6 one step in 64 does."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
sys.path.insert(0, ROOT)

N = 4096
STRIDES = (0, 3, 6)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def medians(legs, n, warm):
    """medians of the legs, run in turn"""
    for _ in range(warm):
        for f in legs:
            f()
    t = [[] for _ in legs]
    for _ in range(n):
        for k, f in enumerate(legs):
            t[k].append(timed(f))
    return [statistics.median(x) for x in t]


def main():
    import numpy as np
    import bhusie_amd as B
    from bhusie_amd import assets, cameras
    args = sys.argv[1:]
    hip = C.CDLL("libamdhip64.so")
    tex = (assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    w, h = cfg.sizes()[-1]
    cam, bh = B.Camera(), B.BlackHole()
    every = (w * h) // N
    rays = np.ascontiguousarray(cameras.pinhole_rays(cam, w, h)[::every][:N])
    assert rays.shape[0] == N
    details = B.RayDetails()
    max_points = [(int(details.max_iterations) >> s) + 2 for s in STRIDES]
    out = {"level": [w, h], "rays": N, "every": every, "strides_log2": list(STRIDES), "max_points": max_points, "library": B.LIB_PATH}
    assert hip.hipSetDevice(0) == 0
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    d_rays, d_out, d_rec, d_pts, d_cnt = (C.c_void_p() for _ in range(5))
    for d, nbytes in ((d_rays, rays.nbytes), (d_out, N * 16), (d_rec, N * 32), (d_pts, N * max(max_points) * 16), (d_cnt, N * 4)):
        assert hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
    assert hip.hipMemcpy(d_rays, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), 1) == 0
    for method, name in ((1, "rk"), (0, "euler")):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex)
        rp.set_uniforms(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=method).uniform())

        def records():
            rp.trace_rays_records_device(d_rays.value, N, d_out.value, d_rec.value, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0

        def paths(s, mp):
            def run():
                rp.trace_rays_paths_device(d_rays.value, N, s, mp, d_out.value, d_rec.value, d_pts.value, d_cnt.value, stream=stream.value)
                assert hip.hipStreamSynchronize(stream) == 0
            return run

        t = medians([records] + [paths(s, mp) for s, mp in zip(STRIDES, max_points)], 30, 5)
        rp.sync()
        cnt = np.zeros(N, np.uint32)
        assert hip.hipMemcpy(C.c_void_p(cnt.ctypes.data), d_cnt, C.c_size_t(cnt.nbytes), 2) == 0
        r = {"records_ms": round(t[0] * 1e3, 4), "points_at_last_stride": int(cnt.sum())}
        for k, s in enumerate(STRIDES):
            r[f"paths_s{s}_ms"] = round(t[1 + k] * 1e3, 4)
            r[f"paths_s{s}_over_records"] = round(t[1 + k] / t[0], 4)
        out[name] = r
        print(name, r, flush=True)
    for d in (d_rays, d_out, d_rec, d_pts, d_cnt):
        hip.hipFree(d)
    hip.hipStreamDestroy(stream)
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
