"""Cost of lensed ray batches (bhray_set_mesh_lensing's BHRAY_LENS_RAYS), one MI355X.  Run by hand:
`python profiles/lensed_rays_cost.py [OUT.json] [--rounds N]`; not a test, and no threshold hangs on it.

The pixel rays of a 1920x1080 frame (`levels = 1`: about 2 M rays, cameras.pinhole_rays), adaptive RK and Euler, the mesh of bench.py --workload mesh
(327 680 triangles) at (4, 0, -8) - in front of the default camera, inside the relativity sphere - three ways:

 lensed_rays   through bhray_trace_rays_device under BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS: the lensed ray-list kernel
 lensed_frame  the same rays as the lensed frame with `levels = 1`: the lensed frame kernel (the same pixels, bit for bit)
 flat_rays     through bhray_trace_rays_device with lensing off: the flat-space mesh ray-list kernel (the mesh inside the sphere is not seen)

Device events on a stream of the script's around each (the batch starts behind the stream and the stream waits for its end; the frame through bhray_wait_stream /
bhray_signal_stream), one warm-up of every shape, then N rounds (9 by default) that alternate the three; the median per leg, in ms and Mrays/s."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
sys.path.insert(0, ROOT)


def main():
    import tempfile
    import numpy as np
    import bhusie_amd as B
    from bhusie_amd import assets, cameras
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = 9
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
        args = [a for a in args if a != sys.argv[sys.argv.index("--rounds") + 1]]
    hip = C.CDLL("libamdhip64.so")
    tex = (assets.temp_lut(256), assets.reference_disk_texture(1000), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    w, h = cfg.sizes()[-1]
    with tempfile.NamedTemporaryFile("w", suffix=".obj", delete=False) as f:
        f.write(assets.icosphere_mesh_obj(7, radius=8.0, bump=0.15, seed=3))
        path = f.name
    model = B.load_model(path)
    os.unlink(path)
    cam, bh = B.Camera(), B.BlackHole()
    rays = np.ascontiguousarray(cameras.pinhole_rays(cam, w, h))
    n = rays.shape[0]
    assert hip.hipSetDevice(0) == 0
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    d_rays, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_rays), C.c_size_t(rays.nbytes)) == 0 and hip.hipMalloc(C.byref(d_out), C.c_size_t(n * 16)) == 0
    assert hip.hipMemcpy(d_rays, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), 1) == 0
    res = {"source": "profiles/lensed_rays_cost.py, one MI355X; device events, median of %d alternating rounds after one warm-up of every shape" % rounds,
           "level": [int(w), int(h)], "rays": int(n), "triangles": int(len(model.arrays()["triangles"])), "mesh_at": [4.0, 0.0, -8.0]}

    def timed(enqueue):
        assert hip.hipEventRecord(ev0, stream) == 0
        enqueue()
        assert hip.hipEventRecord(ev1, stream) == 0
        assert hip.hipStreamSynchronize(stream) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return float(ms.value)

    for method, name in ((1, "rk"), (0, "euler")):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex)
        rp.upload_model(model)
        rp.set_model_transform((4.0, 0.0, -8.0), 1)
        rp.set_uniforms(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=method, model_count=1).uniform())

        def lensed_rays():
            rp.set_mesh_lensing(B.LENS_FRAMES | B.LENS_RAYS)
            return timed(lambda: rp.trace_rays_device(d_rays.value, n, d_out.value, stream=stream.value))

        def lensed_frame():
            rp.set_mesh_lensing(B.LENS_FRAMES | B.LENS_RAYS)

            def enqueue():
                rp.wait_stream(stream.value)
                rp.render()
                rp.signal_stream(stream.value)
            return timed(enqueue)

        def flat_rays():
            rp.set_mesh_lensing(0)
            return timed(lambda: rp.trace_rays_device(d_rays.value, n, d_out.value, stream=stream.value))

        legs = (("lensed_rays", lensed_rays), ("lensed_frame", lensed_frame), ("flat_rays", flat_rays))
        for _, fn in legs:                                   # one warm-up of every shape
            fn()
        rp.sync()
        ts = {k: [] for k, _ in legs}
        for _ in range(rounds):                              # the three alternate
            for k, fn in legs:
                ts[k].append(fn())
        rp.sync()
        res[name] = {k: {"ms": round(statistics.median(v), 4), "mrays_s": round(n / statistics.median(v) / 1e3, 1), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                     for k, v in ts.items()}
        print(name, res[name], flush=True)
        rp.close()
    hip.hipFree(d_rays); hip.hipFree(d_out); hip.hipEventDestroy(ev0); hip.hipEventDestroy(ev1); hip.hipStreamDestroy(stream)
    text = json.dumps(res, indent=1)
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
