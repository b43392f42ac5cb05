"""Cost of the moving observer of stills against the same still without one, and against the parent commit's library.

`python profiles/observer_cost.py [--parent LIBBHRAY_OF_THE_PARENT_COMMIT.so] [--rounds N] [OUT.json]`; not a test.

1920x1080 (`ladder_for_frame((1920, 1080), 3, 1)`), 16-sample box stills of the default scene, RK, the large textures, under the pinhole and the equirect camera, each
with no observer, with beta = (0.5, 0, 0) and aberration only, and with beaming.  The accumulation runs on the ctx's own non-blocking stream, which no call of the
library hands out, so an event recorded by the caller cannot bracket it: a still is timed on the host clock from accum_begin to the return of sync() behind
accum_add(16), the way profiles/still_camera_cost.py times its legs, and divided by 16.  Every leg is a fresh process (median of 9 stills after 3), N processes per
leg in alternating order; with --parent the observer-less legs also run on that library (it has no bhray_accum_set_observer: the same still on the parent commit).
Writes profiles/observer_cost.json (or OUT.json) and prints it."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES, WARM, STILLS = 16, 3, 9
VELOCITY = (0.5, 0.0, 0.0)
CAMERAS = ("pinhole", "equirect")
MODES = ("none", "aberration", "beamed")


def leg(camera, mode):
    sys.path.insert(0, ROOT)
    import bhusie_amd as B
    from bhusie_amd.cameras import StillCamera
    from tests import common as T
    rp = B.RayPass(B.ladder_for_frame((1920, 1080), 3, 1), device=0)
    rp.set_textures(*T.textures(small=False))
    rp.set_uniforms(*T.uniforms(integration_method=1))
    if camera == "equirect":
        rp.accum_set_camera(StillCamera.equirect())
    if mode != "none":
        rp.accum_set_observer(VELOCITY, beaming=(mode == "beamed"))
    ms = []
    for _ in range(WARM + STILLS):
        rp.sync()
        t0 = time.perf_counter()
        rp.accum_begin()
        rp.accum_add(SAMPLES)
        rp.sync()
        ms.append(1e3 * (time.perf_counter() - t0) / SAMPLES)
    rp.close()
    print(json.dumps({"median_ms_per_sample": statistics.median(ms[WARM:]), "min": min(ms[WARM:]), "max": max(ms[WARM:])}))


def run_leg(camera, mode, lib=None):
    env = dict(os.environ)
    if lib:
        env["BHRAY_LIB"] = lib
        env["BHRAY_AB_OLD_BUILD"] = "1"              # symbols the older library lacks are not bound
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", camera, mode], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"leg {camera} {mode} {lib or ''}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv):
    if argv[:1] == ["--leg"]:
        return leg(argv[1], argv[2])
    parent, rounds, out = None, 3, os.path.join(ROOT, "profiles", "observer_cost.json")
    i = 0
    while i < len(argv):
        if argv[i] == "--parent":
            parent = os.path.abspath(argv[i + 1]); i += 2
        elif argv[i] == "--rounds":
            rounds = int(argv[i + 1]); i += 2
        else:
            out = argv[i]; i += 1
    legs = [(c, m, None) for c in CAMERAS for m in MODES] + ([(c, "none", parent) for c in CAMERAS] if parent else [])
    runs = {k: [] for k in legs}
    for _ in range(rounds):
        for k in legs:
            runs[k].append(run_leg(*k)["median_ms_per_sample"])
    result = {"source": "host clock from accum_begin to the return of sync() behind accum_add(16), divided by 16; 1920x1080, levels = 1, default scene, RK, 4096x2048 sky; "
                        f"beta = {VELOCITY}; every leg a fresh process (median of {STILLS} stills after {WARM}), {rounds} processes per leg in alternating order",
              "ms_per_sample": {}}
    for (c, m, lib), v in runs.items():
        name = f"{c}_{m}" + ("_parent_library" if lib else "")
        result["ms_per_sample"][name] = {"median": round(statistics.median(v), 4), "processes": [round(x, 4) for x in v]}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1:])
