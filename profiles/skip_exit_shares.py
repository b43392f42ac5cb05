"""How often does the dense RK march skip its error estimate, and how many rare-region visits only leave?  (profiles/EXPERIMENTS.md R19.1)

The measurement build (`make -C bhusie_amd/csrc shares` -> libbhray_shares.so, -DBHRAY_SHARE_LOG: g_share_log in bhray_kernels.hip) renders the bench frame the way
bench.py does - 1920x1080, 4 ladder levels, 22 frame slots, speculative levels 2, time moving by 1/60 per frame - and its dense no-mesh RK kernels count, per wave-step
of the unified pairs, whether every active lane passes R11.1's bound and the third-order bound, per rare-region visit whether any lane is near the horizon or the disk,
and the lane-steps that pass the third-order bound with an estimate above the controller's threshold (must be 0).  Nothing is timed: the counters cost registers.

  BHRAY_LIB=bhusie_amd/libbhray_shares.so python profiles/skip_exit_shares.py [frames] [frames_in_flight]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhusie_amd as B      # noqa: E402
import bench                # noqa: E402
from bhusie_amd import renderer as R      # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 88
fif = int(sys.argv[2]) if len(sys.argv) > 2 else 22
a = argparse.Namespace(workload="disk", integrator="rk", max_iterations=2000, bvh="reference")
tex, cam, bh, det, model = bench.build_scene(a)
cfg = B.ladder_for_frame((1920, 1080), 3, 4)
rp = B.RayPass(cfg, device=0, frames_in_flight=fif, speculative_levels=2)
rp.set_textures(*tex)
lib = R.lib()
lib.bhray_debug_share_log.argtypes = [C.POINTER(C.c_uint64), C.c_int]
lib.bhray_debug_share_log.restype = C.c_int
out = (C.c_uint64 * 8)()


def block(n, t0):
    for k in range(n):
        det.time = (t0 + k) / 60.0 if hasattr(det, "time") else 0.0
        rp.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())
        rp.render()
    rp.sync()


block(fif, 0)                                            # warm-up: not counted
assert lib.bhray_debug_share_log(out, 1) == 0
w0 = rp.work()
block(frames, fif)
assert lib.bhray_debug_share_log(out, 1) == 0
w1 = rp.work()
steps, calm2, visits, light, calm3, viol3, fail2_lanes, lanes = (int(v) for v in out)
print(f"frames {frames}, slots {fif}; work() before {w0} after {w1}")
print(f"pair wave-steps {steps} ({steps / frames:.0f} per frame); lane-steps {lanes} ({lanes / max(1, steps) / 64:.4f} of the lanes active)")
print(f"  every active lane passes R11.1's bound:        {calm2} = {calm2 / max(1, steps):.4f}   (fail: {1 - calm2 / max(1, steps):.4f}; lane-steps that fail it: {fail2_lanes / max(1, lanes):.4f})")
print(f"  every active lane passes the third-order bound: {calm3} = {calm3 / max(1, steps):.4f}   (fail: {1 - calm3 / max(1, steps):.6f})")
print(f"  lane-steps that pass the third-order bound with e_max above 0.00002: {viol3}")
print(f"rare-region visits {visits} ({visits / max(1, steps) * 16:.3f} per 16 wave-steps); without a lane near the horizon or the disk {light} = {light / max(1, visits):.4f}")
rp.close()
