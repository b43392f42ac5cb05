"""Cost of a sample pass of the accumulation image, one MI355X.  Run by hand: `python profiles/accum_cost.py [OUT.json]`; not a test.

 frame        a `levels = 1` frame of 1920 x 1080 (every pixel traced by the frames' trace kernel): bhray_render + bhray_sync, the yardstick.
 sample pass  bhray_accum_add(S) + bhray_sync over S = 8 samples, divided by S: generate, trace (the ray-list kernels), resolve-and-add.
 trace only   the same trace launches without the other two kernels: S / 2 calls of bhray_trace_rays_device over the rays of samples 0 and 1 resident on the device
              (two samples per launch, as bhray_accum_add groups a frame of this size under the default 2^22 rays per launch), one synchronise, divided by S.
 gen + add    sample pass - trace only: the share of the generator and the resolve-and-add kernel (they run between the trace launches of one stream, so the
              difference also holds the launch gaps - an upper bound on the kernels' own time; the two legs trace different sub-pixel offsets for s >= 2).
Wall clock of enqueue + synchronise, median of 9 after 3.  Both integrators; RK is the number DESIGN.md quotes."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
sys.path.insert(0, ROOT)
S = 8


def med(fn, n=9, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    import numpy as np
    import bhusie_amd as B
    from bhusie_amd import assets
    hip = C.CDLL("libamdhip64.so")
    tex = (assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    npix = int(cfg.frame_w) * int(cfg.frame_h)
    cam, bh = B.Camera(), B.BlackHole()
    out = {"frame": [int(cfg.frame_w), int(cfg.frame_h)], "level": list(cfg.sizes()[-1]), "samples_per_measurement": S, "library": B.LIB_PATH}
    assert hip.hipSetDevice(0) == 0
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    d_rays, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_rays), C.c_size_t(2 * npix * 32)) == 0 and hip.hipMalloc(C.byref(d_out), C.c_size_t(2 * npix * 16)) == 0
    for method, name in ((1, "rk"), (0, "euler")):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex)
        rp.set_uniforms(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=method).uniform())
        rays = np.ascontiguousarray(np.concatenate([rp.accum_sample_rays(0), rp.accum_sample_rays(1)]))
        assert hip.hipMemcpy(d_rays, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), 1) == 0

        def frame():
            rp.render(); rp.sync()

        def sample_pass():
            rp.accum_add(S); rp.sync()

        def trace_only():
            for _ in range(S // 2):
                rp.trace_rays_device(d_rays.value, 2 * npix, d_out.value, stream=stream.value)
            assert hip.hipStreamSynchronize(stream) == 0

        rp.accum_begin()
        t_frame, t_pass, t_trace = med(frame), med(lambda: (rp.accum_begin(), sample_pass())) / S, med(trace_only) / S
        r = {"frame_ms": round(t_frame * 1e3, 4), "sample_pass_ms": round(t_pass * 1e3, 4), "trace_only_ms": round(t_trace * 1e3, 4),
             "gen_add_ms": round((t_pass - t_trace) * 1e3, 4), "gen_add_share": round((t_pass - t_trace) / t_pass, 4),
             "sample_pass_over_frame": round(t_pass / t_frame, 3), "msamples_per_s": round(npix / t_pass / 1e6, 1),
             "hbm_bytes_gen_add_per_sample": npix * (32 + 48)}
        out[name] = r
        print(name, r, flush=True)
        rp.close()
    hip.hipFree(d_rays); hip.hipFree(d_out); hip.hipStreamDestroy(stream)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
