"""Cost of a sample pass of the accumulation image under each still camera, one MI355X.  Run by hand:
`python profiles/still_camera_cost.py [--parent LIBBHRAY_OF_THE_PARENT_COMMIT.so] [--rounds N] [OUT.json]`; not a test.

 sample pass  bhray_accum_begin + bhray_accum_add(S) + bhray_sync over S = 8 samples at 1920 x 1080, RK, divided by S: generate, trace (the ray-list kernels),
              resolve-and-add.  Wall clock, median of 9 after 3, in a child process of its own per leg.
 pinhole      the default camera: accum_gen_kernel, as before still cameras.  With --parent the leg runs alternately under the parent commit's library (BHRAY_LIB) and
              under this tree's, N rounds each (3 by default): the pinhole path must not move beyond the spread of the rounds of one library.
 equirect, fisheye (fov 3.4), lens (radius 0.3, focus 19)   the same pass with bhray_stillcam.hip's generator.  The default scene from the default camera: each
              projection sees another mix of disk, horizon and sky rays, so the legs differ by the trace work of what they look at far more than by their generators -
              the generator's own share is the pinhole row's gen + add (profiles/accum_cost.py) plus two to four sine / cosine pairs per ray."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8
LEGS = ("pinhole", "equirect", "fisheye", "lens")


def med(fn, n=9, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def leg(name):
    """one child: ms per sample pass of one camera under the library BHRAY_LIB names (this tree's by default)"""
    os.environ["GPU_MAX_HW_QUEUES"] = "32"          # as bench.py sets it, before HIP starts
    sys.path.insert(0, ROOT)
    import bhusie_amd as B
    from bhusie_amd import assets
    tex = (assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2))
    cfg = B.ladder_for_frame((1920, 1080), 3, 1)
    rp = B.RayPass(cfg, device=0, frames_in_flight=1)
    rp.set_textures(*tex)
    rp.set_uniforms(B.Camera().uniform(), B.BlackHole().uniform(), B.RayDetails(integration_method=1).uniform())
    if name != "pinhole":                            # (the parent's library has no bhray_accum_set_camera: its leg is the pinhole's)
        from bhusie_amd.cameras import StillCamera
        rp.accum_set_camera({"equirect": StillCamera.equirect(), "fisheye": StillCamera.fisheye(3.4), "lens": StillCamera.pinhole(lens_radius=0.3, focus_distance=19.0)}[name])

    def sample_pass():
        rp.accum_begin(); rp.accum_add(S); rp.sync()

    t = med(sample_pass) / S
    rp.close()
    print(json.dumps({"leg": name, "library": B.LIB_PATH, "sample_pass_ms": round(t * 1e3, 4)}), flush=True)


def child(name, lib=None):
    env = dict(os.environ)
    if lib:
        env["BHRAY_LIB"] = lib
        env["BHRAY_AB_OLD_BUILD"] = "1"              # symbols the older library lacks are not bound
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], env=env, capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise RuntimeError(f"the {name} leg failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["sample_pass_ms"]


def main(argv):
    if len(argv) >= 2 and argv[0] == "--leg":
        return leg(argv[1])
    parent, rounds, out_path = None, 3, None
    i = 0
    while i < len(argv):
        if argv[i] == "--parent":
            parent = os.path.abspath(argv[i + 1]); i += 2
        elif argv[i] == "--rounds":
            rounds = int(argv[i + 1]); i += 2
        else:
            out_path = argv[i]; i += 1
    out = {"frame": [1920, 1080], "samples_per_measurement": S, "method": "rk", "rounds": rounds}
    this, old = [], []
    for _ in range(rounds):                          # alternating: parent, this, parent, this, ...
        if parent:
            old.append(child("pinhole", parent))
        this.append(child("pinhole"))
    out["pinhole_ms"] = {"this": this, "median": statistics.median(this), "spread": max(this) - min(this)}
    if parent:
        out["pinhole_parent_ms"] = {"parent": old, "median": statistics.median(old), "spread": max(old) - min(old)}
        out["pinhole_this_minus_parent_ms"] = round(statistics.median(this) - statistics.median(old), 4)
    for name in LEGS[1:]:
        t = [child(name) for _ in range(rounds)]
        out[name + "_ms"] = {"this": t, "median": statistics.median(t), "spread": max(t) - min(t)}
        print(name, out[name + "_ms"], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
