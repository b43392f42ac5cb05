"""Cost of the still pixel filters, one MI355X.  Run by hand: `python profiles/accum_filter_cost.py [OUT.json]`; not a test.

 box pass       bhray_accum_add(S) + bhray_sync over S = 8 samples of a 1920 x 1080 `levels = 1` frame, divided by S: generate, trace, accum_add_kernel - the
                yardstick (profiles/accum_cost.py's sample pass).
 filtered pass  the same call with bhray_accum_set_filter in force - accum_filter_add_kernel in accum_add_kernel's place - under the Mitchell filter (radius 2) and
                under a tent of radius 1.5.
 extra          filtered pass - box pass: what the 5 x 5 stencil, its halo loads and their repeated resolves cost per sample, launch gaps included.
Wall clock of enqueue + synchronise, median of 9 after 3; the box is measured before and after the filters (`box_again`), which bounds the drift.  Both integrators;
RK is the number DESIGN.md quotes."""
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
    import bhusie_amd as B
    from bhusie_amd import assets
    tex = (assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    npix = int(cfg.frame_w) * int(cfg.frame_h)
    cam, bh = B.Camera(), B.BlackHole()
    out = {"frame": [int(cfg.frame_w), int(cfg.frame_h)], "samples_per_measurement": S, "library": os.path.relpath(B.LIB_PATH, ROOT)}
    legs = (("box", None), ("mitchell_2", B.StillFilter.mitchell(2.0)), ("tent_1.5", B.StillFilter.tent(1.5)), ("box_again", None))
    for method, name in ((1, "rk"), (0, "euler")):
        rp = B.RayPass(cfg, device=0, frames_in_flight=1)
        rp.set_textures(*tex)
        rp.set_uniforms(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=method).uniform())

        def sample_pass():
            rp.accum_begin(); rp.accum_add(S); rp.sync()

        r = {}
        for leg, filt in legs:
            rp.accum_set_filter(filt)
            r[leg + "_pass_ms"] = round(med(sample_pass) / S * 1e3, 4)
        box = 0.5 * (r["box_pass_ms"] + r["box_again_pass_ms"])
        for leg in ("mitchell_2", "tent_1.5"):
            r[leg + "_extra_ms"] = round(r[leg + "_pass_ms"] - box, 4)
            r[leg + "_extra_share"] = round((r[leg + "_pass_ms"] - box) / box, 4)
        r["msamples_per_s_mitchell_2"] = round(npix / r["mitchell_2_pass_ms"] / 1e3, 1)
        out[name] = r
        print(name, r, flush=True)
        rp.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
