"""Cost of the display pass from one rocprofv3 kernel trace.

Render: `rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python profiles/display_cost.py run`
renders 20 frames at 1918x1081 and 20 at 3840x2160, each frame's render synchronised before its display pass so that the pass's 11
kernels run alone.  Summarise: `python profiles/display_cost.py summarise OUT/.../run_kernel_trace.csv` prints, per frame size, the
median over frames 3-20 of the sum of the 11 kernels, their span, and every kernel's median, as JSON (profiles/r07_display_cost.json)."""
import csv
import json
import os
import statistics
import sys

SIZES = ((1918, 1081), (3840, 2160))
POST = ("bloom_kernel", "final_kernel", "fxaa_kernel")


def run():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bhusie_amd as B
    from tests import common as T
    for cfg in (B.ladder_from_base((72, 41), 3, 4), B.ladder_for_frame((3840, 2160), 3, 4)):
        rp = B.RayPass(cfg, device=0)
        rp.set_textures(*T.textures())
        rp.set_uniforms(*T.uniforms(integration_method=1))
        for _ in range(20):
            rp.render(); rp.sync(); rp.resolve_display(); rp.sync()
        rp.close()


def summarise(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    post = [r for r in rows if any(k in r["Kernel_Name"] for k in POST)]
    assert len(post) == 11 * 20 * len(SIZES), len(post)
    out = {"source": "rocprofv3 --kernel-trace, MI355X; each frame's render synchronised before its display pass; medians over frames 3-20",
           "frame_ms_default_bench": 0.40}
    for n, (w, h) in enumerate(SIZES):
        frames = [post[(n * 20 + f) * 11:(n * 20 + f + 1) * 11] for f in range(2, 20)]
        dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
        names = [next(k for k in POST if k in r["Kernel_Name"]) for r in frames[0]]
        per = [statistics.median(dur(f[j]) for f in frames) for j in range(11)]
        sums = [sum(dur(r) for r in f) for f in frames]
        out[f"{w}x{h}"] = {"sum_of_11_kernels_us": {"median": round(statistics.median(sums), 1), "min": round(min(sums), 1), "max": round(max(sums), 1)},
                           "span_first_start_to_last_end_us": round(statistics.median((int(f[-1]["End_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for f in frames), 1),
                           "kernels_us": [f"{i}:{nm} {v:.1f}" for i, (nm, v) in enumerate(zip(names, per))]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else summarise(sys.argv[2])
