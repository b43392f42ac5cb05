"""Cost of ray records, one MI355X.  Run by hand: `python profiles/ray_records_cost.py [OUT.json]`; not a test.

What a record costs is the difference between two kernels over the same rays:

 ray list   bhray_trace_rays_device: the four ray-list kernels of DESIGN.md section 15.  They are the parent commit's kernels - their text, and by the compiler's
            resource report their registers, scratch and occupancy, did not change with the records - so this side of the comparison is the yardstick, not the code
            under test.  (BHRAY_LIB=/path/to/libbhray.so built from the parent commit runs that side from the parent's library itself: give it as
            `--parent-lib PATH` and the script starts itself again for the ray-list side only.)
 records    bhray_trace_rays_records_device: the four record kernels, results and records resident on the device.

 large    Mrays/s of the bench frame's pixel rays (the 1920x1080 frame's only level at `levels = 1`: about 2 M rays, cameras.pinhole_rays), wall clock of enqueue +
          stream synchronisation, median of 9 after 3, the two sides interleaved (ABAB) so that clock drift lands on both.  Both integrators.
 small    latency of a 4 096-ray batch (the first 4 096 of those rays): the device variants (enqueue + synchronise) and the host variants (copy in, trace, copy
          out - the records add a 128 KB copy back), median of 30 after 5.

The records add 32 bytes of stores per ray, on the rare paths and in the epilogue, and nothing to the step loop; the Euler no-mesh record kernel is budgeted for the 5 waves
per SIMD of its twin, the RK one runs at 4 like its twin with 15 more VGPRs."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def med_ab(fa, fb, n, warm):
    """medians of two legs run alternately; fb may be None"""
    for _ in range(warm):
        fa()
        if fb:
            fb()
    ta, tb = [], []
    for _ in range(n):
        ta.append(timed(fa))
        if fb:
            tb.append(timed(fb))
    return statistics.median(ta), (statistics.median(tb) if fb else None)


def main():
    import numpy as np
    import bhusie_amd as B
    from bhusie_amd import assets, cameras
    args = sys.argv[1:]
    parent_lib = None
    if "--parent-lib" in args:
        k = args.index("--parent-lib")
        parent_lib = args[k + 1]
        del args[k:k + 2]
    rays_only = "--ray-list-only" in args
    args = [a for a in args if a != "--ray-list-only"]
    have_records = not rays_only
    hip = C.CDLL("libamdhip64.so")
    tex = (assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    w, h = cfg.sizes()[-1]
    cam, bh = B.Camera(), B.BlackHole()
    rays = np.ascontiguousarray(cameras.pinhole_rays(cam, w, h))
    n = rays.shape[0]
    out = {"level": [w, h], "rays": n, "library": B.LIB_PATH}
    assert hip.hipSetDevice(0) == 0
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    d_rays, d_out, d_rec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_rays), C.c_size_t(rays.nbytes)) == 0 and hip.hipMalloc(C.byref(d_out), C.c_size_t(n * 16)) == 0
    assert hip.hipMalloc(C.byref(d_rec), C.c_size_t(n * 32)) == 0
    assert hip.hipMemcpy(d_rays, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), 1) == 0
    for method, name in ((1, "rk"), (0, "euler")):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex)
        rp.set_uniforms(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=method).uniform())

        def ray_list(count):
            rp.trace_rays_device(d_rays.value, count, d_out.value, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0

        def records(count):
            rp.trace_rays_records_device(d_rays.value, count, d_out.value, d_rec.value, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0

        large = med_ab(lambda: ray_list(n), (lambda: records(n)) if have_records else None, 9, 3)
        small = med_ab(lambda: ray_list(4096), (lambda: records(4096)) if have_records else None, 30, 5)
        host = med_ab(lambda: rp.trace_rays(rays[:4096]), (lambda: rp.trace_rays_records(rays[:4096])) if have_records else None, 30, 5)
        rp.sync()
        r = {"ray_list_ms": round(large[0] * 1e3, 4), "ray_list_mrays_s": round(n / large[0] / 1e6, 1),
             "batch4096_ray_list_device_ms": round(small[0] * 1e3, 4), "batch4096_ray_list_host_ms": round(host[0] * 1e3, 4)}
        if have_records:
            r.update({"records_ms": round(large[1] * 1e3, 4), "records_mrays_s": round(n / large[1] / 1e6, 1), "records_over_ray_list": round(large[1] / large[0], 4),
                      "batch4096_records_device_ms": round(small[1] * 1e3, 4), "batch4096_records_host_ms": round(host[1] * 1e3, 4)})
        out[name] = r
        print(name, r, flush=True)
    hip.hipFree(d_rays); hip.hipFree(d_out); hip.hipFree(d_rec); hip.hipStreamDestroy(stream)
    if parent_lib and not rays_only:            # the ray-list side once more, from the parent commit's own library, in a fresh process
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ray-list-only"], env=dict(os.environ, BHRAY_LIB=parent_lib, BHRAY_AB_OLD_BUILD="1"), capture_output=True, text=True)
        out["parent_library"] = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else {"error": p.stderr[-400:]}
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
