"""Cost and error of an adaptive still next to a uniform one, one MI355X, 1920 x 1080, default scene, RK.  Run by hand:
`python profiles/accum_adaptive_cost.py OUT.json [WORKDIR]`; not a test.  Every step is a fresh child process under a time limit of its own; the first step that fails
or runs out of time ends the run.

 reference  a uniform 1 024-sample still (bhray_accum_add), its mean kept in WORKDIR: what (c) measures against.
 uniform64  (b) a uniform 64-sample still: bhray_accum_begin + bhray_accum_add(64) + bhray_sync, wall clock, median of 5 after 2; (c) its RMS difference from the reference.
 adaptive   (a) an adaptive still min 4 / round 4 / max 64, dark 0.01, at each tolerance of TOLERANCES: bhray_accum_begin + bhray_accum_add_adaptive + bhray_sync, wall
            clock, median of 5 after 2, with the call's rounds and rays and the mean count; (c) its RMS difference from the reference.
 kernels    (d) two adaptive stills at TOLERANCES[1] under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host); of the second one (the first
            warms up), from the trace's timestamps: the summed durations of its selection, generator, add and trace kernels, the span from its first kernel's start to
            its last kernel's end, and the span's remainder - the time no kernel of the still runs: the readback waits of the rounds, launch gaps, the small copies;
            not split further.
RMS: over the r, g, b of all pixels, of the binary32 means, in float64."""
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCES = (0.05, 0.01, 0.002)
MIN, ROUND, MAX, DARK = 4, 4, 64, 0.01
LIMITS = {"reference": 300, "uniform64": 240, "adaptive": 300, "kernels": 300}      # seconds per step


def med(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def ray_pass():
    os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
    sys.path.insert(0, ROOT)
    import bhusie_amd as B
    from bhusie_amd import assets
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    rp = B.RayPass(cfg, device=0, frames_in_flight=1)
    rp.set_textures(assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    rp.set_uniforms(B.Camera().uniform(), B.BlackHole().uniform(), B.RayDetails(integration_method=1).uniform())
    return rp, int(cfg.frame_w) * int(cfg.frame_h)


def rms(a, b):
    import numpy as np
    d = a[..., 0:3].astype(np.float64) - b[..., 0:3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def step(name, work):
    import numpy as np
    rp, npix = ray_pass()
    ref_path = os.path.join(work, "reference_1024.npy")
    out = {}
    if name == "reference":
        rp.accum_begin(); rp.accum_add(1024)
        np.save(ref_path, rp.accum_read())
        out = {"samples": 1024, "pixels": npix}
    elif name == "uniform64":
        def still():
            rp.accum_begin(); rp.accum_add(64); rp.sync()
        m, lo, hi = med(still)
        out = {"ms": round(m * 1e3, 3), "ms_min": round(lo * 1e3, 3), "ms_max": round(hi * 1e3, 3), "rays": 64 * npix,
               "rms_from_reference": rms(rp.accum_read(), np.load(ref_path))}
    elif name == "adaptive":
        ref = np.load(ref_path)
        for tol in TOLERANCES:
            info = {}

            def still():
                rp.accum_begin(); info.update(rp.accum_add_adaptive(MIN, MAX, ROUND, tol, DARK)); rp.sync()
            m, lo, hi = med(still)
            counts = rp.accum_read_counts()
            out[str(tol)] = {"ms": round(m * 1e3, 3), "ms_min": round(lo * 1e3, 3), "ms_max": round(hi * 1e3, 3), "rounds": info["rounds"], "rays": info["rays"],
                             "mean_count": float(counts.mean()), "share_at_min": float((counts == MIN).mean()), "share_at_max": float((counts == MAX).mean()),
                             "rms_from_reference": rms(rp.accum_read(), ref)}
    elif name == "kernels":
        rp.accum_begin(); rp.accum_add_adaptive(MIN, MAX, ROUND, TOLERANCES[1], DARK); rp.sync()       # warm: code objects, staging
        rp.accum_begin(); info = rp.accum_add_adaptive(MIN, MAX, ROUND, TOLERANCES[1], DARK); rp.sync()
        out = {"stills": 2, "rounds": info["rounds"], "rays": info["rays"]}
    rp.close()
    print(json.dumps(out))


def kernel_sums(trace_dir):
    import csv
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, f"no kernel_trace.csv under {trace_dir}"
    names = {"select": "adapt_select_kernel", "gen": "adapt_gen_kernel", "add": "adapt_add_kernel", "trace": "trace_kernel"}
    rows = []
    for r in csv.DictReader(open(paths[0])):
        g = next((k for k, nm in names.items() if nm in r["Kernel_Name"]), None)
        if g:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), g))
    rows.sort()
    assert rows and len(rows) % 2 == 0, f"{len(rows)} dispatches: the two stills must launch the same kernels"
    second = rows[len(rows) // 2:]
    assert [g for _, _, g in second] == [g for _, _, g in rows[:len(rows) // 2]]
    ms = {k: round(sum(e - b for b, e, g in second if g == k) / 1e6, 4) for k in names}
    span = (max(e for _, e, _ in second) - second[0][0]) / 1e6
    return {"second_still": {"kernel_ms": ms, "launches": {k: sum(1 for _, _, g in second if g == k) for k in names}, "span_ms": round(span, 4),
                             "no_kernel_running_ms": round(span - sum(ms.values()), 4)}}


def main():
    out_path = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="bhray_adaptive_cost_")
    os.makedirs(work, exist_ok=True)
    out = {"frame": [1920, 1080], "integrator": "rk", "params": {"min": MIN, "round": ROUND, "max": MAX, "dark": DARK, "tolerances": list(TOLERANCES)},
           "timing": "wall clock of begin + add + bhray_sync, median (min, max) of 5 after 2, one process per step"}
    for name in ("reference", "uniform64", "adaptive", "kernels"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, work]
        if name == "kernels":
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(work, "trace"), "-o", "adaptive", "--"] + cmd
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {LIMITS[name]} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"step {name}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        out[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        if name == "kernels":
            out[name].update(kernel_sums(os.path.join(work, "trace")))
        print(name, json.dumps(out[name]), flush=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        step(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
