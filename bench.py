#!/usr/bin/env python3
"""bench.py — Mrays/s of the geodesic ray-trace pass on N MI355X (BASELINE.json metric).

One step = one frame of the workload through the whole pass (all ladder levels; at N>1 also the
gather of the row tiles to the root GPU and the de-interleave into the frame — both enqueued by
bhray_render inside libbhray: RCCL send/recv + a HIP kernel).  Inputs (uniforms, textures, mesh) are
resident in HBM before the timed region.  value = frame pixels * steps / time.

    python bench.py                       # N=1, configs[1]: 1920x1080 adaptive RK, disk + adaptive grid
    python bench.py --workload mesh       # configs[2]: + BVH mesh (.obj)
    python bench.py --gpus N              # ONE process drives N GPUs through one bhray_ctx (the reference's host model)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N   # one process per GPU, one ctx each;
                                          # torch.distributed (gloo) only carries the barrier and the 128-byte communicator id
    python bench.py --full                # + every secondary figure below (roofline, sustained, latency, literal, hand-off, ...)
    python bench.py --dump-outputs DIR    # + the last timed frame as DIR/frame.npy (float32)

A plain run sets up, warms up (--warmup frames), times ONE block of exactly --steps frames, writes its outputs if asked and prints the
line: metric, value, unit, ms_per_step (= the block's time / --steps), higher_is_better, dtype and the configuration.  Everything else
it measures or checks runs only with --full: the counted frame (traced rays, roofline), the sustained block, the latency / literal /
hand-off / moving-scene / drop-in legs, the CPU baseline and, at N > 1, the byte-for-byte check of the gathered frame.

Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel (trace_kernel; averaged over
all its launches, i.e. the 4 ladder levels, so that it matches the per-kernel average of
`rocprofv3 --kernel-trace --stats`), measured with HIP events recorded on the stream the kernels run
on.  `cpu_baseline` is the CPU oracle (a port of the reference WGSL; the reference itself is
Rust+wgpu and cannot run on this box) on a bounded sample, N=1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# Frames in flight run on separate HIP streams; ROCm maps streams onto 4 hardware queues by default, so 4+ streams
# would serialise pairwise (measured: 8 queues are not enough once the N>1 path adds its side streams and RCCL's).  Must be set before the HIP
# runtime initialises; libbhray only READS it (the host owns the process environment).  32 is the most a process may open on a shared device;
# libbhray gives 30 of them to frame slots, more than the 22 frames in flight of the headline.  Set, not defaulted: an environment that
# exports ROCm's default of 4 would otherwise put the 22 slots on 2 streams and time another pipeline.
os.environ["GPU_MAX_HW_QUEUES"] = "32"

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
VALU_PEAK_TFLOPS = 157.3       # vector FP32 peak
NUM_CUS, CLOCK_GHZ = 256, 2.4  # 256 CUs x 128 FP32 lanes x 2 flop x 2.4 GHz = 157.3 TFLOP/s
FLOPS_PER_STEP = {0: 125.0, 1: 390.0}     # Euler / Cash–Karp, incl. per-step hit tests
FLOPS_NODE_PAIR, FLOPS_TRIANGLE = 60.0, 120.0


def algorithmic_bytes_trace(c: dict) -> float:
    """HBM bytes the trace kernel must move: per traced ray a 4 B queue entry and a
    16 B RGBA32F store; 32 B per disk shading event (2 bilinear taps x 4 texels x 4 B), 16 B per sky
    sample, 64 B per BVH node pair, 124 B per leaf triangle."""
    return (c["traced"] * 20.0 + c["disk_hits"] * 32.0 + c["sky_samples"] * 16.0
            + c["node_pairs"] * 64.0 + c["triangles"] * 124.0)


def algorithmic_bytes_frame(c: dict) -> float:
    """Whole pass: 16 B store per pixel per level, +16 B per copied pixel, +64 B (4 coarse texels)
    per interpolated/refined pixel, + the trace-side taps."""
    refined = c["traced"]
    return (c["pixels"] * 16.0 + c["copied"] * 16.0 + (c["interpolated"] + refined) * 64.0
            + c["disk_hits"] * 32.0 + c["sky_samples"] * 16.0 + c["node_pairs"] * 64.0 + c["triangles"] * 124.0)


def counters_sky_taps(c: dict, frame_pixels: int) -> float:
    """Direction pixels of the final frame = pixels the sky pass has to sample: everything that is not a colour pixel.
    Upper bound from the counters: frame pixels minus the rays that sampled the sky in-kernel or hit something."""
    return float(max(0, frame_pixels - c["sky_samples"]))


def algorithmic_flops(c: dict, method: int) -> float:
    return c["steps"] * FLOPS_PER_STEP[method] + c["node_pairs"] * FLOPS_NODE_PAIR + c["triangles"] * FLOPS_TRIANGLE


def build_scene(args):
    import bhusie_amd as B
    from bhusie_amd import assets
    # disk: the reference's own disk.png regenerated by its asset tool (perlin/src/main.rs restated behind the ABI);
    # LUT and sky are seeded synthetic stand-ins (color.png is an image asset, sky.png is missing from the reference)
    tex = (assets.temp_lut(256), assets.reference_disk_texture(1000), assets.sky_texture(4096, 2048, seed=2))
    cam, bh = B.Camera(), B.BlackHole()
    det = B.RayDetails(integration_method=1 if args.integrator == "rk" else 0, step_size=0.15, max_iterations=args.max_iterations,
                       angle_division_threshold=0.02, time=0.0)
    model = None
    if args.workload == "mesh":
        import tempfile
        obj = assets.icosphere_mesh_obj(7, radius=8.0, bump=0.15, seed=3)          # 327 680 triangles, leaves <= 2
        with tempfile.NamedTemporaryFile("w", suffix=".obj", delete=False) as f:
            f.write(obj)
            path = f.name
        model = B.load_model(path)
        os.unlink(path)
        if args.bvh == "sah":
            model.build_bvh_sah()
        det.model_count = 1
    return tex, cam, bh, det, model


def cpu_baseline(args, tex, cam, bh, det, model):
    """Oracle (port of ray.wgsl) on a bounded sample: one frame of the same workload (frames above 1920x1080 at half size)."""
    import bhusie_amd as B
    from oracle import oracle as O
    fw, fh = args.width, args.height
    if fw * fh > 1920 * 1080:
        fw, fh = max(64, fw // 2), max(36, fh // 2)
    cfg = B.ladder_for_frame((fw, fh), 3, args.levels)
    models = []
    if model is not None:
        models = [model.arrays()]
    sc = O.OracleScene(cam.uniform(), bh.uniform(), det.uniform(), tex[0], tex[1], tex[2], models)
    t0 = time.perf_counter()
    O.render_ladder(sc, cfg.sizes())
    dt = time.perf_counter() - t0
    last = cfg.sizes()[-1]
    return {"value": round(last[0] * last[1] / dt / 1e6, 4), "unit": "Mrays/s", "cores": O.num_threads(), "kind": "port",
            "sample": f"CPU oracle (C restatement of ray.wgsl, OpenMP x{O.num_threads()}), one {last[0]}x{last[1]} frame "
                      f"(ladder {cfg.sizes()[0][0]}x{cfg.sizes()[0][1]} x3 x{args.levels}, same camera/scene, adaptive RK), "
                      f"{dt:.2f} s wall"}


def differing_pixels(a, b) -> int:
    """Pixels of two frames (RGBA32F, or the RGBA16F sky image) that differ: bit for bit, except the SIGN of a NaN.  DESIGN.md section 2,
    "NaN sign": where the shader's arithmetic makes a NaN every build makes it in the same channels, but its sign is specified by neither WGSL
    nor the contract and differs between builds of the same source (the one-slot latency build against the builds of a ctx with several
    frame slots).  A NaN where the other frame has none counts, and so does every other bit.  -1 when the shapes differ."""
    import numpy as np
    if a.shape != b.shape:
        return -1
    word = np.uint16 if a.dtype == np.float16 else np.uint32
    na, nb = np.isnan(a), np.isnan(b)
    wa, wb = a.view(word).copy(), b.view(word).copy()
    wa[na & nb] = 0
    wb[na & nb] = 0
    return int((wa != wb).any(axis=-1).sum())


DUMP_BYTES = 48 << 20                            # --dump-outputs: a frame above this is written as a seeded sample of its pixels


def dump_outputs(out_dir: str, rp, sky: bool = False) -> None:
    """What the caller of the timed path receives from its last frame: the RGBA32F frame (bhray_read_hdr; at N > 1 the gathered frame on
    the root), or with BHRAY_F_GATHER_SKY the RGBA16F sky image widened to float32.  The same arguments give the same inputs (seeded
    textures, the same frame clock), so two builds can be compared array for array.  A frame above DUMP_BYTES keeps a fixed seeded sample
    of its pixels (frame_sample.npy, pixels x 4) and their flat indices (frame_sample_index.npy, float64: exact)."""
    import numpy as np
    img = rp.read_sky().astype(np.float32) if sky else rp.read_hdr()
    name = "sky" if sky else "frame"
    os.makedirs(out_dir, exist_ok=True)
    if img.nbytes <= DUMP_BYTES:
        np.save(os.path.join(out_dir, name + ".npy"), img)
        return
    flat = img.reshape(-1, img.shape[-1])
    n = DUMP_BYTES // (flat.shape[1] * flat.itemsize + 8)
    idx = np.sort(np.random.default_rng(20261016).choice(flat.shape[0], size=n, replace=False))
    np.save(os.path.join(out_dir, name + "_sample.npy"), np.ascontiguousarray(flat[idx]))
    np.save(os.path.join(out_dir, name + "_sample_index.npy"), idx.astype(np.float64))


def auto_frames_per_batch(args, world: int) -> int:
    """Frames per launch.  A launch lasts at least as long as its longest ray (~0.4 ms) however few rays it holds, and about
    16 launches run concurrently, so the rays per launch decide the throughput once a GPU renders only a row tile of the
    frame: batch enough frames to give a launch about two full 1920x1080 frames' worth of rows (measured, emulated per rank:
    N=8 0.0675 ms per frame at 16 frames per batch against 0.0745 at 8; N=4 best at 8, N=2 at 4; N=1: no batching).  A timed
    block needs several batches to overlap one batch's coarse (latency-bound) launches with another's last level: never more than a
    QUARTER of a block (since a batch's coarse launches are dealt out thinly, EXPERIMENTS R4.14: 1080p over 8 / 4 GPUs, 20-frame blocks, 5 frames
    per batch 0.0848 / 0.1302 ms per frame against 0.0877 / 0.1482 at 10; long blocks still want 10-16)."""
    if world <= 1 and args.width * args.height >= 1920 * 1080:
        return 1
    share = max(1.0, args.height / max(1, world)) * args.width           # pixels of one GPU's share of a frame
    want = max(1, min(16, round(2.5 * 1920 * 1080 / share)))
    cap = max(1, args.steps // 4)
    if want >= cap:
        return int(cap)
    # a short timed block in batches of EQUAL size (an odd last batch is a launch chain of its own with little in it): the divisor of the
    # block length nearest to the wanted size, the larger one on a tie (3840x2160 over 8 GPUs, 20-frame blocks: 4 batches of 5 frames
    # 0.2386 ms per frame, 5 of 4: 0.2604, 3 of 7 / 7 / 6: 0.2556 - profiles/r04_emu_knobs.txt)
    divs = [d for d in range(1, cap + 1) if args.steps % d == 0]
    return int(min(divs, key=lambda d: (abs(d - want), -d)))


def share_bounds(launcher, bounds, world: int):
    """Every rank of a launcher renders the same calibration frame and computes the same slab bounds; rank 0's are broadcast all the same,
    so that one bit of difference between two GPUs' counters can never split the ranks over two partitions."""
    if launcher.world <= 1:
        return [int(v) for v in bounds]
    import struct
    blob = launcher.broadcast_bytes(struct.pack("<%dI" % (world + 1), *bounds) if launcher.rank == 0 else None, 4 * (world + 1))
    return list(struct.unpack("<%dI" % (world + 1), blob))


def reweigh_by_probe(cfg, work, bounds, probe_ms, frame_h: int):
    """The feedback round of the balanced partition: every level row's modelled work times (its slab's measured time / the mean time).
    The owner of a level row is the slab that owns the frame row it lies under (coarse rows near a bound serve two slabs: either weight will do)."""
    import numpy as np
    mean = sum(probe_ms) / len(probe_ms)
    hl = cfg.level_h[cfg.levels - 1]
    out = []
    for a in work:
        yy = (np.arange(len(a)) * (hl - 1.0) / max(1, len(a) - 1) - cfg.crop_y).clip(0, frame_h - 1)
        owner = np.searchsorted(np.asarray(bounds[1:-1]), yy, side="right")
        out.append((np.asarray(a, dtype=np.float64) * np.asarray(probe_ms)[owner] / mean).astype(np.uint64))
    return out


def rebalance_over_launcher(launcher, costs_extras, cur, row_weight, frame_h: int):
    """One round of the balance for one process per GPU: every rank hands in the costs of ITS partition (bhray_get_partition_costs: zeros for the
    others), the launcher's channel sums them, every rank runs the library's arithmetic (bhray_rebalance_slabs) on the same numbers and gets the same
    bounds.  Returns what bhray_rebalance reports; the caller applies the bounds (bhray_set_partition) when `applied` says so."""
    import bhusie_amd as B
    cost, extra = costs_extras
    n = len(cost)
    tot = launcher.reduce(list(cost) + list(extra), op="sum")
    cost, extra = tot[:n], tot[n:]
    new, pred = B.rebalance_slabs(frame_h, cur, cost, row_weight, extra_ms=extra)
    before = max(c_ + e_ for c_, e_ in zip(cost, extra))
    apply = list(new) != list(cur) and pred < 0.98 * before
    return {"applied": bool(apply), "slab_row0": list(new) if apply else list(cur), "part_cost": cost, "extra_cost": extra, "slowest_before": before, "slowest_predicted": pred}


def launcher_env():
    """(world, rank, local_rank) of a one-process-per-GPU launcher (torchrun), or (1, 0, 0)."""
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


class stdout_to_stderr:
    """stdout carries exactly ONE JSON line.  Libraries that print banners on it (RCCL when a communicator is created, gloo when a
    process group connects) do so through C stdio, block-buffered on a pipe: redirect fd 1 to fd 2 for the duration and flush C
    stdio before restoring it."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        import ctypes
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


class GatherFailed(RuntimeError):
    """N > 1: a block's gather failed on some rank (every rank raises it together: block())"""


class Launcher:
    """The launcher's plumbing for the one-process-per-GPU mode: a barrier, a max / sum over ranks and the broadcast of the
    128-byte communicator id.  torch.distributed over gloo on CPU tensors — the pixels never pass through it: the gather of the
    row tiles is RCCL inside libbhray, enqueued by bhray_render."""

    def __init__(self, world: int, rank: int):
        self.world, self.rank, self.dist = world, rank, None
        if world > 1:
            import torch
            import torch.distributed as dist
            self.torch, self.dist = torch, dist
            with stdout_to_stderr():
                dist.init_process_group("gloo")
                dist.barrier()

    def barrier(self):
        if self.dist:
            self.dist.barrier()

    def reduce(self, values, op="sum", dtype="float64"):
        if not self.dist:
            return list(values)
        t = self.torch.tensor(list(values), dtype=getattr(self.torch, dtype))
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX if op == "max" else self.dist.ReduceOp.SUM)
        return t.tolist()

    def broadcast_bytes(self, blob, n: int) -> bytes:
        if not self.dist:
            return blob
        t = self.torch.tensor(list(blob) if self.rank == 0 else [0] * n, dtype=self.torch.uint8)
        self.dist.broadcast(t, src=0)
        return bytes(t.tolist())

    def close(self):
        if self.dist:
            with stdout_to_stderr():
                self.dist.barrier()
                self.dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--workload", choices=["disk", "mesh"], default="disk")
    ap.add_argument("--bvh", choices=["reference", "sah"], default="reference", help="mesh workload: the reference-identical midpoint builder, or the flagged SAH builder")
    ap.add_argument("--integrator", choices=["rk", "euler"], default="rk", help="rk = the metric's adaptive RK (Cash-Karp); euler = the reference's UI default")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--max-iterations", type=int, default=2000)
    ap.add_argument("--stripe-rows", type=int, default=27)
    ap.add_argument("--partition", choices=["auto", "stripes", "balanced", "library"], default="auto",
                    help="N>1: how frame rows are dealt to the GPUs.  stripes = interleaved stripes of --stripe-rows rows; library = contiguous slabs that the ctx "
                         "balances ITSELF (bhray_rebalance: the steps its trace waves issue + the pixels it classifies, per partition; a few rounds during the warm-up, "
                         "no calibration frame, no counting build, no second ctx); balanced = the host-side calibration of rounds 3-4 (a calibration frame rendered whole "
                         "with counters -> bhray_balance_slabs -> timed feedback rounds, every partition in a ctx of its own); auto = library, balanced when one rank is emulated")
    ap.add_argument("--rebalance-rounds", type=int, default=5, help="--partition library: warm-up blocks, each followed by bhray_rebalance, before the timed region")
    ap.add_argument("--sequence", choices=["auto", "none", "time", "orbit"], default="auto",
                    help="secondary leg: a MOVING scene, the reference host's real workload - `time += dt` every frame (mod.rs:382; the disk texture turns), and with "
                         "`orbit` a camera strafing around the hole at the UI's default speed (scene/mod.rs: 7.5 units/s at 60 frames/s) - rendered by the ladder and by "
                         "BHRAY_F_TEMPORAL, every frame of one block verified byte-identical between the two.  auto = orbit when the extra legs run")
    ap.add_argument("--no-partition-feedback", dest="partition_feedback", action="store_false", help="--partition balanced: bounds from the work model alone (no timed feedback round)")
    ap.add_argument("--partition-feedback-temporal", action="store_true", help="--partition balanced: the feedback probes render with BHRAY_F_TEMPORAL (a host that runs the partitions in that mode: "
                    "its cost per pixel row differs from the ladder's, so do the balanced bounds); the `sequence` leg then shows that host's ranks")
    ap.add_argument("--partition-feedback-rounds", type=int, default=2, help="--partition balanced: timed feedback rounds (each re-weights every slab's rows by its measured time and balances again)")
    ap.add_argument("--static-time", action="store_true", help="every timed frame with time = 0 (rounds 1-3); default: time += 1/60 per frame, as the reference's render loop does (mod.rs:382)")
    ap.add_argument("--sustained-steps", type=int, default=200, help="frames of the one long block timed after the --steps blocks (0 = skip): the rate without pipeline fill and drain")
    ap.add_argument("--frames-in-flight", type=int, default=22, help="frame slots (one HIP stream each); 20-22 saturate the device (22: +1.3 %% sustained, +2.5 %% on 20-frame "
                    "blocks over 20); the library serves larger requests with 22 (beyond that the HIP runtime stalls intermittently, measured)")
    ap.add_argument("--speculative-levels", type=int, default=-1, help="-1 = auto: 2 when the ladder has at least 3 levels")
    ap.add_argument("--superset-levels", type=int, default=0, help="bhray_config.superset_levels (the last U levels traced in one launch over a conservative superset)")
    ap.add_argument("--frames-per-batch", type=int, default=-1, help="frames covered by every launch (bhray_config.frames_per_batch); -1 = auto")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--gather-root", type=int, default=0, help="N>1: partition whose GPU receives every frame (the display GPU)")
    ap.add_argument("--devices", default="", help="N>1 without a launcher: HIP device of every partition, e.g. 0,1,2,3 (default 0..N-1); a repeated device "
                    "(0,0,0,0) is the functional test of the N>1 path on a one-GPU box (tiles travel as RCCL send/recv-to-self)")
    ap.add_argument("--process-model", choices=["auto", "single", "multi"], default="auto",
                    help="N>1: 'single' = ONE process drives the N GPUs through one bhray_ctx (what the reference's one-thread host does; the default "
                         "without a launcher); 'multi' = one process per GPU, each with its own ctx, same in-library RCCL gather (the default under torchrun)")
    ap.add_argument("--verify", action="store_true", help="N>1: after the timed region compare the gathered frame with a frame rendered whole on one GPU, byte for byte")
    ap.add_argument("--emulate-world", type=int, default=0, help="single process renders only one rank's row tiles of an N-way partition (sizing experiments)")
    ap.add_argument("--emulate-rank", type=int, default=0, help="with --emulate-world: which rank's row tiles to render")
    ap.add_argument("--readback", choices=["none", "async", "sync"], default="none", nargs="?", const="async",
                    help="hand every frame of the timed region to host memory (PCIe-inclusive; never the headline): async = bhray_read_hdr_async into a ring of "
                         "pinned buffers (an SDMA copy in stream order behind each frame's kernels; the other slots render meanwhile), sync = bhray_read_hdr after every render")
    ap.add_argument("--eval", choices=["contract", "literal", "fma"], default="contract",
                    help="integrator evaluation of the timed region: contract = the default kernels (DESIGN.md §2), literal = BHRAY_F_LITERAL (ray.wgsl operator "
                         "by operator), fma = BHRAY_F_EVAL_FMA (the text with fused multiply-add contraction only)")
    ap.add_argument("--literal", action="store_true", help="shorthand for --eval literal")
    ap.add_argument("--gather-sky", action="store_true", help="N>1: BHRAY_F_GATHER_SKY - every partition runs the sky pass over its own rows and the RGBA16F image is what is "
                    "gathered (half the bytes over xGMI); the verification then compares sky images")
    ap.add_argument("--no-verify", action="store_true", help="N>1: skip the byte-for-byte comparison of the gathered frame with the frame rendered whole (on by default)")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the isolated / latency / literal / hand-off legs (profiling runs)")
    ap.add_argument("--min-seconds", type=float, default=0.0, help="0 (default): ONE timed block of exactly --steps frames.  Above 0: the block is repeated until "
                    "this much time has been measured and the MEDIAN block is reported (a 20-step block lasts ~10 ms: one block alone is at the mercy of a clock ramp; "
                    "the committed bench lines under profiles/ were taken with 0.5)")
    ap.add_argument("--pmc-json", default="", help="PMC summary (profiles/summarize.py) collected from THIS command in the same session: enables valu.issue")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline: the counted frame (traced rays, roofline, valu), "
                    "the sustained block, the latency / literal / hand-off / moving-scene / drop-in legs, the CPU baseline and, at N > 1, the verification "
                    "of the gathered frame (each still subject to its own --no-* option)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed block, write the frame the timed path delivered last as DIR/frame.npy "
                    "(float32, rows x width x RGBA; DIR/sky.npy with --gather-sky); a frame above 48 MB is written as a fixed seeded sample of its pixels")
    args = ap.parse_args()
    if args.literal:
        args.eval = "literal"
    if args.readback is None:
        args.readback = "async"
    eval_kw = {"contract": {}, "literal": {"literal": True}, "fma": {"eval_fma": True}}[args.eval]
    if args.gpus > 1 and not args.no_verify and args.full:
        args.verify = True
    if not args.full:                             # a plain run: set-up, warm-up, the timed block, the outputs, the line
        args.sustained_steps = 0
        args.no_extra_legs = True
        args.no_cpu_baseline = True
        args.sequence = "none"

    lw, lrank, llocal = launcher_env()
    if lw > 1 and lw != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={lw}")
    n_gpus = max(1, args.gpus)
    model_ = args.process_model
    if model_ == "auto":
        model_ = "multi" if lw > 1 else "single"
    if model_ == "multi" and lw == 1 and n_gpus > 1:
        raise SystemExit("--process-model multi needs a launcher (torchrun --nproc-per-node N)")
    launcher = Launcher(lw, lrank)
    # who renders: 'multi' — every rank, its own partition; 'single' — one process (rank 0 of a launcher, the others only keep
    # the launcher's barriers company)
    active = model_ == "multi" or lrank == 0
    import bhusie_amd as B

    tex, cam, bh, det, model = build_scene(args)
    cfg = B.ladder_for_frame((args.width, args.height), 3, args.levels)
    devices = None
    if n_gpus > 1 and model_ == "single":
        devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(n_gpus))
        if len(devices) != n_gpus:
            raise SystemExit(f"--devices lists {len(devices)} devices, --gpus is {n_gpus}")
    comm_id = None
    if n_gpus > 1 and model_ == "multi":
        comm_id = launcher.broadcast_bytes(B.comm_unique_id() if lrank == 0 else None, 128)
    spec = args.speculative_levels
    if spec < 0:
        spec = 2 if args.levels >= 3 else 0      # levels 0 and 1 traced in one launch (fewer dependent launches; identical pixels)
    fpb = args.frames_per_batch
    if fpb < 0:
        fpb = auto_frames_per_batch(args, args.emulate_world or n_gpus)

    slabs = [None]                               # --partition balanced: slab_row0[0..N] (filled below from a calibration frame)

    def make_pass(whole=False, **kw):
        """whole=True: the undivided frame on one GPU (counters of the algorithmic work, --verify, the isolated leg)."""
        if whole or n_gpus == 1:
            part = dict(device=(llocal if model_ == "multi" else (devices[0] if devices else 0)))
            if args.emulate_world and not whole:
                part.update(row_rank=args.emulate_rank, row_world=args.emulate_world, slab_row0=slabs[0])
        elif model_ == "single":
            part = dict(devices=devices, gather_root=args.gather_root, slab_row0=slabs[0])
        else:
            part = dict(device=llocal, row_rank=lrank, row_world=lw, comm_id=comm_id, gather_root=args.gather_root, slab_row0=slabs[0])
        rp = B.RayPass(cfg, stripe_rows=args.stripe_rows, **part, **kw)
        rp.set_textures(*tex)
        if model is not None:
            rp.upload_model(model)
        rp.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())
        return rp

    # --partition balanced: one calibration frame, rendered whole with the speculative levels the partitions will use, tells where
    # the work lies (iterations per level row); the slab bounds equalise it (pure host arithmetic inside libbhray).  Every rank of a
    # launcher renders the same frame and gets the same bounds; rank 0's are broadcast all the same.
    world_parts = args.emulate_world or n_gpus
    partition = args.partition if args.partition != "auto" else ("balanced" if args.emulate_world else "library")
    if partition == "library" and args.emulate_world:
        raise SystemExit("--partition library balances a ctx that holds every partition (or a rank of a communicator); with --emulate-world use --partition balanced")
    partition_d = None
    if world_parts > 1 and partition == "library":
        slabs[0] = [args.height * p_ // world_parts for p_ in range(world_parts + 1)]        # equal slabs; the ctx moves them during the warm-up (below)
        partition_d = {"mode": "balanced slabs (bhray_rebalance)", "slab_row0_at_create": list(slabs[0])}
    if world_parts > 1 and partition == "balanced":
        t0 = time.perf_counter()
        rpc = make_pass(whole=True, counters=True, frames_in_flight=1, speculative_levels=spec)
        rpc.render()
        work = rpc.row_work()
        rpc.close()
        b = share_bounds(launcher, B.balance_slabs(cfg, work, world_parts), world_parts)
        slabs[0] = b
        b0_ = b
        # Feedback rounds (--partition-feedback-rounds).  Ray iterations are the work MODEL; what a GPU pays per modelled iteration differs by a few per cent
        # between slabs (the hole's rows: long rays, disk shading, emptier waves; the sky's: short uniform rays) - measured 0.51-0.57 of
        # the VALU peak over the eight slabs of the 1080p frame.  So every partition is timed alone for a moment with the bounds just
        # found and the SAME block length as the timed region (no gather: a ctx of its own), each slab's rows are re-weighted by its time
        # against the mean, and the bounds are balanced again.  One process per GPU: every rank times its own partition and the launcher
        # sums the vectors; one process, N GPUs (and --emulate-world): the partitions are timed one after the other.
        probe_ms = None
        probes_ = []
        w_cur = work
        for round_ in range(max(1, args.partition_feedback_rounds) if args.partition_feedback else 0):
            b = slabs[0]
            mine = [0.0] * world_parts
            todo = [lrank] if (model_ == "multi" and lw > 1) else (list(range(world_parts)) if lrank == 0 else [])
            for q in todo:
                dev_q = llocal if (model_ == "multi" and lw > 1) else (devices[q] if devices else 0)
                probe_kw = dict(temporal=True) if args.partition_feedback_temporal else dict(speculative_levels=spec)
                pq = B.RayPass(cfg, device=dev_q, row_rank=q, row_world=world_parts, slab_row0=b, frames_in_flight=args.frames_in_flight,
                               frames_per_batch=fpb, **probe_kw, **eval_kw)
                pq.set_textures(*tex)
                if model is not None:
                    pq.upload_model(model)
                pq.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())
                if args.partition_feedback_temporal:          # every frame slot position must have held a frame before (its prediction comes from it)
                    for _ in range(min(args.frames_in_flight, 22) * fpb + fpb):
                        pq.render()
                ts_ = []
                for k_ in range(1 + max(3, min(40, int(400 / max(1, args.steps))))):
                    pq.sync(); t1 = time.perf_counter()
                    for _ in range(args.steps):
                        pq.render()
                    pq.sync(); ts_.append(time.perf_counter() - t1)
                pq.close()
                mine[q] = sorted(ts_[1:])[len(ts_[1:]) // 2] / args.steps * 1e3
            probe_ms = launcher.reduce(mine, op="sum") if lw > 1 else mine
            probes_.append([round(v, 5) for v in probe_ms])
            if min(probe_ms) <= 0:
                break
            w_cur = reweigh_by_probe(cfg, w_cur, b, probe_ms, args.height)          # cumulative: every round corrects the weights the last bounds came from
            slabs[0] = share_bounds(launcher, B.balance_slabs(cfg, w_cur, world_parts), world_parts)
        partition_d = {"mode": "balanced slabs", "slab_row0": slabs[0], "slab_row0_from_the_work_model": b0_, "probe_ms_per_frame": probes_[-1] if probes_ else None, "probe_ms_per_frame_by_round": probes_ or None,
                       "calibration_ms": round((time.perf_counter() - t0) * 1e3, 1),
                       "note": "contiguous row slabs: bounds from bhray_balance_slabs over bhray_get_row_work of ONE calibration frame rendered whole, then feedback rounds (--partition-feedback-rounds) - every "
                               "partition timed alone for a few blocks, its rows re-weighted by its time against the mean, balanced again; all before the timed region"}
    elif world_parts > 1 and partition == "stripes":
        partition_d = {"mode": "interleaved stripes", "stripe_rows": args.stripe_rows}
    counters = None
    rank_counters = None                         # --emulate-world: the work of the ONE rank this process renders (incl. its redundant coarse rows)
    if lrank == 0 and args.full:                 # algorithmic work of the frame: an untimed render of the undivided frame
        rpc = make_pass(whole=True, counters=True, frames_in_flight=1)
        rpc.render()
        counters = rpc.counters()
        rpc.close()
        if args.emulate_world:
            rpc = make_pass(counters=True, frames_in_flight=1)
            rpc.render()
            rank_counters = rpc.counters()
            rpc.close()
    rp = info = None
    fallback = None
    main_kw = dict(timing="sparse", frames_in_flight=args.frames_in_flight, speculative_levels=spec, frames_per_batch=fpb, superset_levels=args.superset_levels, **eval_kw)
    if args.gather_sky and n_gpus > 1:
        main_kw["gather_sky"] = True
    failed = ""
    if active:
        try:
            with stdout_to_stderr():         # RCCL prints a version banner when a communicator is created
                rp = make_pass(**main_kw)
        except B.BhrayError as e:
            if not (n_gpus > 1 and model_ == "multi"):
                raise
            failed = f"rank {lrank}: {e}"
    if n_gpus > 1 and model_ == "multi" and launcher.reduce([1.0 if failed else 0.0])[0] > 0:
        # a rank could not join the communicator (all ranks learn it here): one process drives the N GPUs instead, if it sees them
        if failed:
            print("bench: one process per GPU failed (" + failed + "); falling back to one process, N GPUs", file=sys.stderr)
        if rp is not None:
            rp.close()
            rp = None
        fallback = failed or "another rank could not create its ctx"
        model_ = "single"
        active = lrank == 0
        devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(n_gpus))
        if active:
            with stdout_to_stderr():
                rp = make_pass(**main_kw)
    if rp is not None:
        info = rp.gather_info()

    issue = [0.0]
    # The reference advances RayDetails.time every frame (mod.rs:382: the disk texture turns with time * rotation_speed); so do the timed frames.
    # The uniform bytes of 240 consecutive frames (4 s at 60 frames/s, then the loop repeats) are made before anything is timed.
    frame_clock = [0]
    u_time = None
    if not args.static_time:
        u_time = [(cam.uniform(), bh.uniform(), B.RayDetails(integration_method=det.integration_method, step_size=det.step_size, max_iterations=det.max_iterations,
                                                           angle_division_threshold=det.angle_division_threshold, time=k_ / 60.0, model_count=det.model_count).uniform()) for k_ in range(240)]

    def run_frames(p, n, readback, ring):
        """n frames through pass p; readback 'async': every frame is handed to a ring of pinned host buffers on the library's copy
        streams (the consumer takes a buffer back - waits for its copy - before it is reused); 'sync': bhray_read_hdr per frame."""
        tickets = [None] * len(ring) if ring else []
        flush_at = [int(v) for v in os.environ.get("BENCH_FLUSH_AT", "").split(",") if v]      # (experiment: uneven batches inside a block)
        for i in range(n):
            if i in flush_at:
                p.flush()
            if readback == "async":
                k = i % len(ring)
                if tickets[k] is not None:
                    p.wait_read(tickets[k])
            if u_time is not None:
                p.set_uniforms(*u_time[frame_clock[0] % len(u_time)])
                frame_clock[0] += 1
            p.render()
            if readback == "async":
                tickets[k] = p.read_hdr_async(ring[k])
            elif readback == "sync":
                p.read_hdr()
        t_issue = time.perf_counter()
        for t in tickets:
            if t is not None:
                p.wait_read(t)
        return t_issue

    ring = []
    if args.readback == "async" and rp is not None and info["root_is_local"]:
        nrows = args.height if not args.emulate_world else len(rp.local_rows())
        ring = [B.PinnedFrame(nrows, args.width) for _ in range(args.frames_in_flight + 2)]     # (--readback async is PCIe-bound: run it with --frames-in-flight 4..8)

    def block(n):
        """n frames through the pass, bracketed by a barrier + device synchronisation on both sides; max over ranks.
        N > 1: a gather that fails on ANY rank (a collective error, the library's watchdog - BHRAY_COMM_TIMEOUT_MS - on a peer that never posts) is
        learnt by EVERY rank over the launcher's channel behind the closing barrier and raised as GatherFailed everywhere: nobody waits at a
        barrier for a rank that has left."""
        launcher.barrier()
        err = None
        t0 = time.perf_counter()
        try:
            if rp is not None:
                rp.sync()
            t0 = time.perf_counter()
            if rp is not None:
                if os.environ.get("BENCH_TEST_GATHER_FAILS") and n_gpus > 1 and gather_attempts[0] <= int(os.environ["BENCH_TEST_GATHER_FAILS"]):
                    raise B.BhrayError(-9, "BENCH_TEST_GATHER_FAILS: a gather failure injected by the test")
                t_issue = run_frames(rp, n, args.readback if (ring or args.readback == "sync") else "none", ring)
                issue[0] = t_issue - t0                  # host time to enqueue the block (all GPUs of this process): every bhray_set_uniforms + bhray_render, up to the return of the last one
                rp.sync()
        except B.BhrayError as e:
            if n_gpus == 1:
                raise
            err = e
        launcher.barrier()
        el, iss, bad = launcher.reduce([time.perf_counter() - t0, issue[0], 1.0 if err is not None else 0.0], op="max")
        issue[0] = iss                                   # one process per GPU: the slowest rank's
        if bad > 0:
            raise GatherFailed(f"rank {lrank}: {err}" if err is not None else "the gather failed on another rank")
        return el

    gather_attempts = [1]
    gather_fallbacks = []

    def warm_up():
      if partition_d is not None and partition == "library":
          # The ctx balances itself: a block of frames, then bhray_rebalance (every rank of a launcher calls it: the partitions' numbers travel over the
          # ctx's own communicator) - the work its kernels counted for the frames its slots hold decides the next bounds.  All before the timed region.
          t0_ = time.perf_counter()
          hist_ = []
          import numpy as np
          w_rows_ = np.zeros(args.height)                  # one process per GPU: the row weights bhray_rebalance would keep inside the ctx
          for _ in range(max(1, args.rebalance_rounds)):
              block(max(args.warmup, args.steps, 2 * fpb))
              if rp is not None and model_ == "multi" and lw > 1:
                  # one process per GPU: every rank's own numbers (bhray_get_partition_costs: local, no collective), summed over the launcher's
                  # channel (gloo, like the barrier), the library's arithmetic on every rank, the same bounds set on every rank.  (bhray_rebalance
                  # does the same with one all-gather over the ctx's communicator; the launcher's channel is the one the CPU tests can exercise.)
                  h_ = rebalance_over_launcher(launcher, rp.partition_costs(), rp.get_partition(), w_rows_, args.height)
                  if h_["applied"]:
                      rp.set_partition(h_["slab_row0"])
                  hist_.append(h_)
              else:
                  reb_err = None
                  if rp is not None:
                      try:
                          hist_.append(rp.rebalance())
                      except B.BhrayError as e_:
                          reb_err = e_
                  if launcher.reduce([1.0 if reb_err is not None else 0.0], op="max")[0] > 0:      # (every rank of a launcher learns it, also the ones that only keep the barriers company)
                      raise GatherFailed(f"bhray_rebalance on rank {lrank}: {reb_err}" if reb_err is not None else "bhray_rebalance failed on another rank")
          if rp is not None:
              slabs[0] = list(hist_[-1]["slab_row0"])          # (a later ctx of this run - the sustained leg's - starts from the balanced bounds)
              partition_d.update({"slab_row0": hist_[-1]["slab_row0"], "rounds": len(hist_), "applied": sum(1 for h_ in hist_ if h_["applied"]),
                                  "part_cost_wave_steps_per_frame": [round(v, 1) for v in hist_[-1]["part_cost"]], "root_extra_cost": round(max(hist_[-1]["extra_cost"]), 1),
                                  "imbalance_first_last": [round(h_["slowest_before"] / max(1e-9, (sum(h_["part_cost"]) + sum(h_["extra_cost"])) / len(h_["part_cost"])), 3) for h_ in (hist_[0], hist_[-1])],
                                  "calibration_ms": round((time.perf_counter() - t0_) * 1e3, 1),
                                  "note": "contiguous row slabs from equal bounds; bhray_rebalance after each of a few warm-up blocks: cost of a partition = integrator steps its trace waves issued "
                                          "+ classified pixels at their price (+ on the root the pixels it receives and de-interleaves); all before the timed region, in the timed ctx itself"})
      block(args.warmup)

    # N > 1: a gather that fails during the warm-up (an RCCL error, the library's watchdog, bhray_rebalance's all-gather) must not cost the run its number
    # - nor its time: VERDICT r5 item 4.  Every rank learns it (block()); the ctx is dropped and a simpler one is tried, in this order: the same process
    # model with interleaved stripes (no rebalance: nothing but the gather itself uses the communicator), then - one process per GPU only - one process
    # driving the N GPUs (ncclCommInitAll instead of a bootstrap over the launcher's id).  The line says which one `value` comes from (gather.fallbacks).
    while True:
        try:
            warm_up()
            break
        except GatherFailed as e:
            what = f"attempt {gather_attempts[0]} ({model_}, {partition_d['mode'] if partition_d else 'one partition'}): {e}"
            print("bench: the gather failed during the warm-up - " + what, file=sys.stderr)
            gather_fallbacks.append(what[:600])
            for b_ in ring:
                b_.free()
            ring = []
            if rp is not None:
                try:
                    rp.close()
                except B.BhrayError:
                    pass
                rp = None
            gather_attempts[0] += 1
            if partition_d is not None and "stripes" not in partition_d["mode"]:
                partition = "stripes"; slabs[0] = None
                partition_d = {"mode": "interleaved stripes", "stripe_rows": args.stripe_rows, "fallback_from": "balanced slabs: " + what[:200]}
            elif model_ == "multi":
                model_ = "single"; active = lrank == 0
                fallback = what[:300]
                devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(n_gpus))
            else:
                print("bench: FAILED: no gather configuration left to fall back to", file=sys.stderr)
                launcher.close()
                sys.exit(5)
            failed3 = ""
            if n_gpus > 1 and model_ == "multi":
                comm_id = launcher.broadcast_bytes(B.comm_unique_id() if lrank == 0 else None, 128)
            if active:
                try:
                    with stdout_to_stderr():
                        rp = make_pass(**main_kw)
                except B.BhrayError as e2:
                    failed3 = f"rank {lrank}: {e2}"
            if launcher.reduce([1.0 if failed3 else 0.0])[0] > 0:
                print("bench: FAILED: the fallback ctx could not be created" + (" (" + failed3 + ")" if failed3 else ""), file=sys.stderr)
                launcher.close()
                sys.exit(5)
            info = rp.gather_info() if rp is not None else None
            if args.readback == "async" and rp is not None and info["root_is_local"]:
                ring = [B.PinnedFrame(args.height, args.width) for _ in range(args.frames_in_flight + 2)]
    if rp is not None:
        rp.timing()                              # reset the event aggregation
    blocks, issues = [], []
    while True:
        blocks.append(block(args.steps))
        issues.append(issue[0])
        go = [1.0 if (sum(blocks) < args.min_seconds and len(blocks) < 500) else 0.0]
        if launcher.reduce(go, op="max")[0] == 0.0:
            break
    elapsed = sorted(blocks)[len(blocks) // 2]   # the median block of exactly --steps frames
    if args.dump_outputs and rp is not None and info["root_is_local"]:
        dump_outputs(args.dump_outputs, rp, sky=bool(main_kw.get("gather_sky")))        # before any leg renders another frame into the ctx
    # one long block with the same ctx: what the pass sustains once the pipeline is full (a 20-frame block is fill + drain of a ladder
    # whose dependent launches last as long as their longest rays, however few rays a GPU's row tiles hold: DESIGN.md §4.5)
    sustained = None
    sus_fpb = fpb
    if args.sustained_steps > 0 and args.frames_per_batch < 0:
        import copy
        a2 = copy.copy(args); a2.steps = args.sustained_steps
        sus_fpb = auto_frames_per_batch(a2, args.emulate_world or n_gpus)          # a long block wants bigger batches than a 20-frame one
        if n_gpus > 1 and model_ == "multi":
            sus_fpb = fpb          # one process per GPU: no second communicator just for this leg (an untested collective start-up is not worth a secondary number)

    def sustained_leg(same_ctx: bool):
        block(min(args.sustained_steps, 40))
        sus = sorted(block(args.sustained_steps) for _ in range(3))[1]
        return {"steps": args.sustained_steps, "ms_per_step": round(sus / args.sustained_steps * 1e3, 5),
                "mrays_per_s": round(args.width * args.height * args.sustained_steps / sus / 1e6, 3), "blocks": 3, "reported": "median block",
                "frames_per_batch": sus_fpb if not same_ctx else fpb,
                "note": "ONE block of this many frames, same bracketing as `value`: the sustained rate; `value` is the driver's --steps block" +
                        ("" if same_ctx else "; a ctx of its own with the batch size the rule gives a block of this length (same partition, same everything else)")}
    if args.sustained_steps > 0 and sus_fpb == fpb:
        sustained = sustained_leg(True)
    # host time to enqueue one frame, from the MEDIAN --steps block (the block `value` comes from) - not from whatever block ran last (round 4
    # took it from the sustained block, whose "issue" time includes blocking on full frame slots).  A --steps block never fills the slots.
    host_issue_ms = issues[sorted(range(len(blocks)), key=lambda i_: blocks[i_])[len(blocks) // 2]] / max(1, args.steps) * 1e3
    tm = rp.timing() if rp is not None else None

    verified = None
    if args.verify and n_gpus > 1 and rp is not None and info["root_is_local"]:
        ref_rp = make_pass(whole=True, frames_in_flight=1, **eval_kw)
        ref_rp.render()
        sky_mode = bool(main_kw.get("gather_sky"))
        if sky_mode:
            ref_rp.resolve_sky()
        ref = ref_rp.read_sky() if sky_mode else ref_rp.read_hdr()
        ref_rp.close()
        import numpy as np
        rp.set_uniforms(cam.uniform(), bh.uniform(), det.uniform())       # the same frame through the partitioned ctx (the timed frames had their own times)
        rp.render()
        got = rp.read_sky() if sky_mode else rp.read_hdr()
        bad = differing_pixels(got, ref)          # (the timed ctx and this one-slot ctx run different builds: a NaN's sign may differ)
        if bad != 0:
            print(f"bench: rank {lrank}: the gathered frame differs from the frame rendered whole on one GPU ({bad} pixels)", file=sys.stderr)
            sys.exit(3)
        verified = 1
    for b_ in ring:
        b_.free()
    if rp is not None:                           # the legs below want the device to themselves (and its hardware queues)
        rp.close()
        rp = None
    if args.sustained_steps > 0 and sus_fpb != fpb:
        # the long block in a ctx of its own (bigger batches).  One process per GPU: a new communicator, so a new id from rank 0; every
        # rank learns whether all of them got their ctx before anyone renders into it
        failed2 = ""
        if n_gpus > 1 and model_ == "multi":
            comm_id = launcher.broadcast_bytes(B.comm_unique_id() if lrank == 0 else None, 128)
        if active:
            try:
                with stdout_to_stderr():
                    rp = make_pass(**dict(main_kw, frames_per_batch=sus_fpb))
            except B.BhrayError as e:
                failed2 = f"rank {lrank}: {e}"
        if launcher.reduce([1.0 if failed2 else 0.0])[0] > 0:
            if failed2:
                print("bench: the sustained leg's ctx could not be created (" + failed2 + "); leg skipped", file=sys.stderr)
        else:
            block(args.warmup)
            sustained = sustained_leg(False)
        if rp is not None:
            rp.close()
            rp = None
    # the same kernels with nothing else on the device (one frame at a time): clean per-launch durations and the latency of
    # ONE frame — the reference host's operating mode (desired_maximum_frame_latency 2, it presents every frame it renders)
    iso = iso_sky = None
    lat_ms = None
    lat_modes = None
    literal_d = handoff_d = None
    if lrank == 0 and not args.no_extra_legs:
        rp1 = make_pass(whole=True, timing=True, frames_in_flight=1, speculative_levels=spec)
        for _ in range(3):
            rp1.render()
        rp1.sync(); rp1.timing()
        lat = []
        for _ in range(12):
            t0 = time.perf_counter()
            rp1.render(); rp1.sync()
            lat.append(time.perf_counter() - t0)
        lat_ms = sorted(lat)[len(lat) // 2] * 1e3
        iso = rp1.timing()
        # the pass that follows the ray pass in the reference (sky.wgsl): HBM-bound, reported next to the ray pass
        for _ in range(10):
            rp1.render(); rp1.resolve_sky(); rp1.sync()
        iso_sky = rp1.timing()
        rp1.close()
        # one frame at a time with temporal speculation (BHRAY_F_TEMPORAL, levels <= 4): the previous frame's traced set is traced in
        # one launch, the ladder only fixes up what it missed.  Static camera = perfect prediction (best case); moving camera = the
        # reference's interactive use (an orbit step of 0.02 rad + 0.3 units per frame: every frame's prediction is one frame old).
        if args.levels <= 4:
            import math
            rpt = make_pass(whole=True, frames_in_flight=1, temporal=True)

            def timed(uniform_list):
                ts = []
                for u_ in uniform_list:
                    rpt.set_uniforms(*u_)
                    t0 = time.perf_counter()
                    rpt.render(); rpt.sync()
                    ts.append(time.perf_counter() - t0)
                return sorted(ts)[len(ts) // 2] * 1e3
            static_u = (cam.uniform(), bh.uniform(), det.uniform())
            timed([static_u] * 3)
            t_static = timed([static_u] * 12)
            path = []
            for i in range(14):
                a = 0.02 * i
                pos = (19.0 * math.sin(a), 0.3 * i, -19.0 * math.cos(a))
                n = math.sqrt(sum(v * v for v in pos))
                path.append((B.Camera(position=pos, forward=tuple(-v / n for v in pos)).uniform(), bh.uniform(), det.uniform()))
            timed(path[:2])
            t_moving = timed(path[2:])
            rpt.close()
            t_s3 = None
            if args.levels >= 4:                 # the plain ladder with its three coarse levels traced in one launch: fewer dependent launches, +190 k rays
                rp3 = make_pass(whole=True, frames_in_flight=1, speculative_levels=3)
                ts3 = []
                for i in range(15):
                    t0 = time.perf_counter()
                    rp3.render(); rp3.sync()
                    if i >= 3:
                        ts3.append(time.perf_counter() - t0)
                rp3.close()
                t_s3 = sorted(ts3)[len(ts3) // 2] * 1e3
            lat_modes = {"ladder_speculative_levels_%d" % spec: round(lat_ms, 4), "ladder_speculative_levels_3": round(t_s3, 4) if t_s3 else None,
                         "temporal_static_camera": round(t_static, 4),
                         "temporal_moving_camera": round(t_moving, 4),
                         "note": "host wall time of bhray_render + bhray_sync, median of 12 frames, one frame in flight, nothing else on the device; "
                                 "every mode delivers the same pixels (tests/test_gpu_temporal.py)"}
    if lrank == 0 and not args.no_extra_legs and n_gpus == 1 and not args.emulate_world and args.eval == "contract":
        # (a) what the LITERAL kernel costs (BHRAY_F_LITERAL: ray.wgsl's integrator operator by operator, bit-identical to the literal
        # oracle): the same timed blocks, a few of them, and one frame at a time.  (b) the third evaluation (BHRAY_F_EVAL_FMA) likewise.
        def short_leg(**kw):
            p_ = make_pass(whole=True, frames_in_flight=args.frames_in_flight, speculative_levels=spec, **kw)
            ts_ = []
            for i_ in range(6):
                p_.sync(); t0_ = time.perf_counter()
                for _ in range(args.steps):
                    p_.render()
                p_.sync(); ts_.append(time.perf_counter() - t0_)
            p_.close()
            p_ = make_pass(whole=True, frames_in_flight=1, speculative_levels=spec, **kw)
            l_ = []
            for i_ in range(10):
                t0_ = time.perf_counter(); p_.render(); p_.sync(); l_.append(time.perf_counter() - t0_)
            p_.close()
            blk = sorted(ts_[1:])[len(ts_[1:]) // 2]
            return {"mrays_per_s": round(args.width * args.height * args.steps / blk / 1e6, 2), "ms_per_step": round(blk / args.steps * 1e3, 5),
                    "latency_ms_one_frame_in_flight": round(sorted(l_[2:])[len(l_[2:]) // 2] * 1e3, 4), "blocks": 5, "steps_per_block": args.steps}
        literal_d = short_leg(literal=True)
        literal_d["note"] = ("BHRAY_F_LITERAL: the integrator of ray.wgsl:401-480 operator by operator (no fused multiply-add, no reassociation), bit-identical to the literal "
                             "oracle on every direction pixel (tests/test_gpu_literal.py); same frames in flight, same timed blocks as `value`")
        literal_d["eval_fma"] = short_leg(eval_fma=True)
        # (a') how far the headline kernel's frame is from the literal kernel's, in THIS run: one frame of each (same uniforms, the frame `value` starts
        # from), the metric of BASELINE.json's north_star - max over channels of |contract - literal| / max(|literal|, 1e-3) - and the pixels beyond 1e-4
        # (a pixel whose class differs counts as beyond).  tests/test_gpu_literal.py bounds the same numbers; DESIGN.md section 2 says what they are.
        def literal_distance():
            import numpy as np
            fr_ = []
            for kw_ in (dict(), dict(literal=True)):
                p_ = make_pass(whole=True, frames_in_flight=1, speculative_levels=spec, **kw_)
                p_.render(); fr_.append(p_.read_hdr()); p_.close()
            con_, lit_ = fr_
            same_ = con_[..., 3] == lit_[..., 3]
            with np.errstate(invalid="ignore"):
                e_ = (np.abs(con_ - lit_) / np.maximum(np.abs(lit_), 1e-3)).max(axis=-1)
            ok_ = same_ & np.isfinite(e_)
            beyond_ = int((~same_).sum()) + int((e_[ok_] > 1e-4).sum())
            return {"pixels_beyond_1e-4": beyond_, "pixels": int(same_.size), "fraction_beyond_1e-4": round(beyond_ / float(same_.size), 6),
                    "class_differences": int((~same_).sum()), "nan_pixels_in_different_places": int((np.isnan(con_).any(axis=-1) != np.isnan(lit_).any(axis=-1)).sum()),
                    "median_rel_err": float(np.median(e_[ok_])), "max_rel_err": float(e_[ok_].max()),
                    "metric": "max over channels of |contract - literal| / max(|literal|, 1e-3), this run's two frames (the frame `value` starts from)"}
        literal_d["distance_of_the_headline_kernel"] = literal_distance()
        # (c) the hand-off to a consumer on another device (the reference's SkyPipeline samples the output as a wgpu texture): every frame
        # copied to pinned host memory.  async = bhray_read_hdr_async (SDMA copy in stream order behind the frame's kernels); sync = the
        # naive binding (bhray_read_hdr after every render).
        def handoff_leg(mode):
            nslots = min(args.frames_in_flight, 4) if mode == "async" else 1       # a PCIe-bound pipeline: a few slots hide the ladder's latency, more only queue
            p_ = make_pass(whole=True, frames_in_flight=nslots, speculative_levels=spec)
            ring_ = [B.PinnedFrame(args.height, args.width) for _ in range(nslots + 2)] if mode == "async" else []
            ts_ = []
            for i_ in range(5):
                p_.sync(); t0_ = time.perf_counter()
                run_frames(p_, args.steps, mode, ring_)
                p_.sync(); ts_.append(time.perf_counter() - t0_)
            for b_ in ring_:
                b_.free()
            p_.close()
            blk = sorted(ts_[1:])[len(ts_[1:]) // 2]
            return {"mrays_per_s": round(args.width * args.height * args.steps / blk / 1e6, 2), "ms_per_step": round(blk / args.steps * 1e3, 5),
                    "host_gb_per_s": round(args.width * args.height * 16 * args.steps / blk / 1e9, 2)}
        def handoff_sky_leg():
            nslots = min(args.frames_in_flight, 10)          # 16.6 MB per frame: the link is no longer the limit, more slots hide the ladder's latency
            p_ = make_pass(whole=True, frames_in_flight=nslots, speculative_levels=spec)
            ring_ = [B.PinnedFrame(args.height, args.width, channels16=True) for _ in range(nslots + 2)]
            ts_ = []
            for i_ in range(5):
                tk_ = [None] * len(ring_)
                p_.sync(); t0_ = time.perf_counter()
                for f_ in range(args.steps):
                    k_ = f_ % len(ring_)
                    if tk_[k_] is not None:
                        p_.wait_read(tk_[k_])
                    p_.render(); p_.resolve_sky()
                    tk_[k_] = p_.read_sky_async(ring_[k_])
                for t_ in tk_:
                    if t_ is not None:
                        p_.wait_read(t_)
                p_.sync(); ts_.append(time.perf_counter() - t0_)
            for b_ in ring_:
                b_.free()
            p_.close()
            blk = sorted(ts_[1:])[len(ts_[1:]) // 2]
            return {"mrays_per_s": round(args.width * args.height * args.steps / blk / 1e6, 2), "ms_per_step": round(blk / args.steps * 1e3, 5),
                    "host_gb_per_s": round(args.width * args.height * 8 * args.steps / blk / 1e9, 2),
                    "note": "ray pass + sky pass (sky.wgsl) in the library, the RGBA16F result handed over: half the bytes of the RGBA32F hand-off"}
        h_async, h_sync = handoff_leg("async"), handoff_leg("sync")
        h_sky = handoff_sky_leg()
        handoff_d = {"mrays_per_s_with_handoff": h_async["mrays_per_s"], "async_pinned": h_async, "async_pinned_sky_rgba16f": h_sky, "sync_read_hdr_one_frame_at_a_time": h_sync,
                     "bytes_per_frame": args.width * args.height * 16,
                     "note": "every frame of the timed blocks delivered to pinned host memory (PCIe-inclusive; never `value`): bhray_read_hdr_async (an SDMA copy in stream order behind each frame's kernels) "
                             "with 4 frame slots into a ring of 6 pinned buffers, the consumer takes each buffer back before it is reused; zero-copy alternative: "
                             "bhray_import_external_fd + bhray_bind_output (INTEGRATION.md §3)"}
    # A moving scene (--sequence): what the reference host renders - every frame has its own `time` (mod.rs:382: the disk texture turns
    # with time * rotation_speed) and, with `orbit`, its own camera (a strafe around the hole at the UI's default 7.5 units/s, 60 frames/s,
    # looking at it).  Rendered (a) by the ladder as in `value` and (b) with BHRAY_F_TEMPORAL - one launch traces what the frame that held
    # this slot position before had to trace, the ladder fixes up what that prediction missed - which a static scene could never show
    # honestly (its prediction would be perfect).  Same timed blocks as `value`; one block of frames is verified byte for byte between (a) and (b).
    seq_kind = args.sequence
    if seq_kind == "auto":
        seq_kind = "orbit" if (not args.no_extra_legs and n_gpus == 1 and args.levels <= 4) else "none"
    sequence_d = None
    if seq_kind != "none" and lrank == 0 and n_gpus == 1 and args.levels <= 4 and args.eval == "contract":
        import math
        import numpy as np
        dt_ = 1.0 / 60.0
        step_ang = 7.5 * dt_ / 19.0                              # scene/mod.rs:32,49: camera_move_speed * dt sideways, at the default distance from the hole

        def seq_uniform(i):
            if seq_kind == "orbit":
                a_ = step_ang * i
                pos_ = (19.0 * math.sin(a_), 0.0, -19.0 * math.cos(a_))
                cam_ = B.Camera(position=pos_, forward=(-math.sin(a_), 0.0, math.cos(a_)))
            else:
                cam_ = cam
            det_ = B.RayDetails(integration_method=det.integration_method, step_size=det.step_size, max_iterations=det.max_iterations,
                                angle_division_threshold=det.angle_division_threshold, time=dt_ * i, model_count=det.model_count)
            return cam_.uniform(), bh.uniform(), det_.uniform()

        # warm-up: every frame slot must have held a frame before the timed blocks (BHRAY_F_TEMPORAL predicts a frame from the frame that
        # held its slot position before; a slot's first frame has no prediction and is the plain ladder)
        nwarm_ = max(args.warmup, 8, min(args.frames_in_flight, 22) * fpb + fpb)
        nseq_ = nwarm_ + 7 * args.steps
        useq_ = [seq_uniform(i) for i in range(nseq_)]           # the uniform bytes of every frame, made before anything is timed

        def seq_leg(**kw):
            """blocks of --steps consecutive frames of the sequence (every frame its own uniforms), median block; then one frame at a time"""
            p_ = make_pass(frames_in_flight=args.frames_in_flight, frames_per_batch=fpb, **kw)
            i_ = 0
            for _ in range(nwarm_):
                p_.set_uniforms(*useq_[i_]); p_.render(); i_ += 1
            ts_ = []
            for _b in range(7):
                p_.sync(); t0_ = time.perf_counter()
                for _ in range(args.steps):
                    p_.set_uniforms(*useq_[i_]); p_.render(); i_ += 1
                p_.sync(); ts_.append(time.perf_counter() - t0_)
            p_.close()
            p_ = make_pass(frames_in_flight=1, **kw)
            l_ = []
            for k_ in range(14):
                p_.set_uniforms(*useq_[k_]); t0_ = time.perf_counter(); p_.render(); p_.sync(); l_.append(time.perf_counter() - t0_)
            p_.close()
            blk = sorted(ts_[1:])[len(ts_[1:]) // 2]
            return {"mrays_per_s": round(args.width * args.height * args.steps / blk / 1e6, 2), "ms_per_step": round(blk / args.steps * 1e3, 5),
                    "latency_ms_one_frame_in_flight": round(sorted(l_[2:])[len(l_[2:]) // 2] * 1e3, 4)}
        lad_ = seq_leg(speculative_levels=spec)
        tmp_ = seq_leg(temporal=True)
        # verification: the temporal ctx exactly as timed (slots, batches: a slot position's prediction is slots x batch frames old) against the ladder
        pt_ = make_pass(frames_in_flight=min(args.frames_in_flight, 4), frames_per_batch=1, temporal=True)
        pl_ = make_pass(frames_in_flight=1, speculative_levels=spec)
        nver_, bad_ = 0, 0
        for i_ in range(max(args.steps, 12)):
            u_ = seq_uniform(i_)
            pt_.set_uniforms(*u_); pl_.set_uniforms(*u_)
            pt_.render(); pl_.render()
            a_, b_ = pt_.read_hdr(), pl_.read_hdr()
            nver_ += 1
            if differing_pixels(a_, b_) != 0:           # (four slots against one: different builds, a NaN's sign may differ)
                bad_ += 1
        pt_.close(); pl_.close()
        if bad_:
            print(f"bench: {bad_} of {nver_} frames of the moving sequence differ between BHRAY_F_TEMPORAL and the ladder", file=sys.stderr)
            sys.exit(3)
        sequence_d = {"kind": seq_kind, "dt": dt_, "camera": ("strafe around the hole, %.5f rad per frame at radius 19, looking at it" % step_ang) if seq_kind == "orbit" else "static",
                      "ladder": lad_, "temporal": tmp_, "verified_frames": nver_, "frames_in_flight": args.frames_in_flight, "frames_per_batch": fpb,
                      "emulated_rank": ([args.emulate_rank, args.emulate_world] if args.emulate_world else None),
                      "note": "every frame of the timed blocks has its own time (and camera); `ladder` = the pass as in `value` (speculative levels %d), `temporal` = BHRAY_F_TEMPORAL; "
                              "mrays_per_s counts the WHOLE frame's pixels also when one rank of an N-way partition is emulated (divide ms_per_step of N = 1 by it for the rank's scaling); "
                              "verified_frames = consecutive frames compared byte for byte between the two" % spec}
    # The drop-in path INTEGRATION.md §3 prescribes, timed from the C++ host program over the header-only mirror of the reference's
    # surface (bhusie_amd/bhray_render --dropin: one thread, `time += dt` every frame, every frame handed to pinned host memory): the
    # naive binding (bhray_read_hdr after every render), and the shim's form - pass() enqueues the frame + the library's sky pass + the
    # copy of its RGBA16F image, finish() hands over the previous frame - with 2 frames in flight (the swap chain's frame latency).
    dropin = None
    if lrank == 0 and not args.no_extra_legs and n_gpus == 1 and not args.emulate_world and args.eval == "contract" and args.workload == "disk":
        import subprocess
        exe = os.path.join(ROOT, "bhusie_amd", "bhray_render")
        try:
            r_ = subprocess.run([exe, "--dropin", "60"] + (["--rk"] if args.integrator == "rk" else []), capture_output=True, text=True, timeout=300)
            line = [l_ for l_ in r_.stdout.splitlines() if l_.startswith("{")]
            if r_.returncode == 0 and line:
                dropin = json.loads(line[-1])
                dropin["note"] = ("bhusie_amd/bhray_render --dropin (C++, host/renderer.hpp: Renderer::render_handoff = the Rust shim's update + pass + finish): the reference-native "
                                  "72x41 x3 x4 ladder, time += 1/60 per frame, one host thread, every frame delivered to pinned host memory; PCIe-inclusive, never `value`")
            else:
                dropin = {"error": (r_.stderr or r_.stdout)[-300:]}
        except Exception as e_:                     # the line must not depend on the C++ program
            dropin = {"error": repr(e_)}
    if lrank == 0:
        pixels = args.width * args.height
        ms_per_step = elapsed / args.steps * 1e3
        value = pixels * args.steps / elapsed / 1e6
        if args.full:
            # dominant kernel: trace_kernel, from the launches of the GPU that delivers the frame (at N>1 it traced only its row
            # tiles: its share of the algorithmic bytes is taken as rows/frame rows of the whole frame's)
            # `avg_ms` = the kernel's EXECUTION span (first block start -> last block end, stamped by the kernel on the device clock): what
            # rocprofv3 --kernel-trace reports as its duration.  HIP events around the launch (`enq_ms`) also contain the time the launch
            # waits for room beside the persistent kernels of the other frames in flight - reported next to it, not used for the roofline.
            launches = max(1, tm.trace_launches)
            enq_ms = tm.trace_ms / launches
            exec_launches = int(tm.trace_exec_launches)
            avg_ms = tm.trace_exec_ms / exec_launches if exec_launches else enq_ms
            frames = max(1, tm.frames)
            share = 1.0
            if n_gpus > 1:       # the rows the delivering GPU traced itself (its tiles do not travel)
                wire_row_ = args.width * 8 if main_kw.get("gather_sky") else (3 * args.width + (args.width + 31) // 32) * 4
                share = info["bytes_received_per_frame"] and 1.0 - info["bytes_received_per_frame"] / float(wire_row_ * args.height)
            work = rank_counters if rank_counters is not None else counters      # --emulate-world: this rank's own rays, not the whole frame's
            bytes_per_launch = algorithmic_bytes_trace(work) * share * frames / launches
            achieved_gbs = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            method = 1 if args.integrator == "rk" else 0
            flops_per_frame = algorithmic_flops(work, method)     # per GPU when emulating one rank of N
            # HBM traffic of the same kernel from the committed PMC passes (profiles/collect.sh: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE,
            # separate passes of the default command); the instruction-issue view only from a PMC summary of THIS session (--pmc-json)
            traffic, traffic_note, valu_issue = None, None, None
            default_cmd = args.workload == "disk" and n_gpus == 1 and args.integrator == "rk" and (args.width, args.height) == (1920, 1080) and args.eval == "contract" and not args.emulate_world
            # the committed PMC summaries (profiles/collect.sh) of the four profiled commands
            prof_wl = None
            if n_gpus == 1 and args.eval == "contract" and not args.emulate_world:
                key = (args.workload, args.integrator, args.width, args.height)
                prof_wl = {("disk", "rk", 1920, 1080): "default", ("disk", "euler", 1920, 1080): "euler", ("mesh", "rk", 1920, 1080): "mesh", ("disk", "rk", 3840, 2160): "4k"}.get(key)
            tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json" if prof_wl in (None, "default") else f"pmc_traffic_{prof_wl}.json")
            default_cmd = prof_wl is not None
            if os.path.exists(tpath) and default_cmd:
                tj = json.load(open(tpath))
                traffic = round(tj["bytes_per_launch_corrected"], 1)
                traffic_note = (f"committed PMC passes of this command (profiles/{tj['tag']}_pmc{'' if prof_wl == 'default' else '_' + prof_wl}.json, not this run): FETCH_SIZE {tj['FETCH_SIZE_KB_per_launch']:.0f} KB x2 "
                                f"(gfx950 correction) + WRITE_SIZE {tj['WRITE_SIZE_KB_per_launch']:.0f} KB per launch; raw sum {tj['bytes_per_launch_raw']:.0f} B")
            issue_src = args.pmc_json if (args.pmc_json and os.path.exists(args.pmc_json)) else (tpath if os.path.exists(tpath) else "")
            if issue_src and default_cmd:
                tj = json.load(open(issue_src))
                if "valu_insts_per_launch" in tj:
                    insts_frame = tj["valu_insts_per_launch"] * launches / frames
                    issue_cap = NUM_CUS * 4 * (CLOCK_GHZ * 1e9 / 2.0) * (ms_per_step * 1e-3)
                    valu_issue = {"valu_wave_insts_per_frame": round(insts_frame, 0), "frac_of_issue_rate": round(insts_frame / issue_cap, 4),
                                  "active_lane_fraction": round(tj.get("valu_active_lane_fraction", 0.0), 4) or None,
                                  "source": os.path.relpath(issue_src, ROOT) + ("" if args.pmc_json else " (committed PMC pass of the default command on this tree, not this run)"),
                                  "note": "SQ_INSTS_VALU of trace_kernel (PMC pass of this command) x launches per frame of this run, / "
                                          "(256 CUs x 4 SIMDs x 1.2e9 wave-instructions/s x wall time per frame)"}
            valu_tflops = flops_per_frame / (ms_per_step * 1e-3) / 1e12 / n_gpus    # per GPU: (whole-frame | this rank's) flops / wall per frame / GPUs
            # the same fraction from the COMMITTED rocprofv3 --kernel-trace --stats summary of this command (profiles/<tag>_kernel_stats*.csv):
            # the kernel's average duration there, so that a reader need not reconcile the in-run span with the CSV
            frac_from_profiles = None
            if prof_wl is not None:
                import csv
                import glob
                cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_kernel_stats" + ("" if prof_wl == "default" else "_" + prof_wl) + ".csv")))
                if cands:
                    with open(cands[-1]) as fcsv:
                        rows_ = [r_ for r_ in csv.DictReader(fcsv) if "trace_kernel" in r_["Name"]]
                    if rows_:
                        calls_ = sum(int(r_["Calls"]) for r_ in rows_)
                        avg_ns_ = sum(float(r_["TotalDurationNs"]) for r_ in rows_) / max(1, calls_)
                        gbs_ = bytes_per_launch / (avg_ns_ * 1e-9) / 1e9
                        frac_from_profiles = {"source": os.path.relpath(cands[-1], ROOT), "avg_launch_ms": round(avg_ns_ * 1e-6, 5), "calls": calls_,
                                              "achieved": round(gbs_, 4), "frac": round(gbs_ / HBM_PEAK_GBS, 6),
                                              "note": "algorithmic bytes per launch of THIS run / the trace kernel's average duration in the committed rocprofv3 summary of the same command "
                                                      "(a profiled run: fewer launches overlap than un-profiled, DESIGN.md §5)"}
            iso_d = None
            if iso is not None and iso.trace_launches:
                iso_ms = iso.trace_ms / iso.trace_launches
                iso_bytes = algorithmic_bytes_trace(counters) * iso.frames / iso.trace_launches
                iso_gbs = iso_bytes / (iso_ms * 1e-3) / 1e9
                iso_d = {"avg_launch_ms": round(iso_ms, 5), "launches": int(iso.trace_launches), "achieved": round(iso_gbs, 4),
                         "frac": round(iso_gbs / HBM_PEAK_GBS, 6),
                         "level_trace_ms": [round(iso.level_trace_ms[i] / max(1, iso.frames), 5) for i in range(args.levels)],
                         "valu_tflops": round(flops_per_frame * iso.frames / (iso.trace_ms * 1e-3) / 1e12, 4),
                         "note": "same kernels, one frame in flight, nothing else on the device (matches rocprofv3 --stats of `bench.py --frames-in-flight 1`)"}
            sky_d = None
            if iso_sky is not None and iso_sky.sky_launches:
                sky_ms = iso_sky.sky_ms / iso_sky.sky_launches
                sky_bytes = pixels * 24.0 + counters_sky_taps(counters, pixels) * 16.0
                sky_d = {"kernel": "sky_kernel (sky.wgsl, rgba32f -> rgba16f)", "avg_launch_ms": round(sky_ms, 5), "launches": int(iso_sky.sky_launches),
                         "algorithmic_bytes_per_launch": sky_bytes, "achieved": round(sky_bytes / (sky_ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(sky_bytes / (sky_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         "note": "16 B read + 8 B written per pixel + 16 B of sky texels per direction pixel; not part of `value`"}
            gather_d = None
            if n_gpus > 1:
                g = max(1, tm.gathers)
                gather_d = {"transport": "RCCL grouped ncclSend/ncclRecv inside libbhray (dlopen'ed librccl %d), enqueued by bhray_render" % info["rccl_version"],
                            "process_model": ("one process, %d GPUs, one bhray_ctx" % n_gpus) if model_ == "single" else "one process per GPU (launcher), one bhray_ctx each",
                            "process_model_fallback": fallback,
                            "fallbacks": gather_fallbacks or None,
                            "devices": devices, "comm_ranks": info["comm_ranks"], "root": info["root"],
                            "bytes_received_per_frame": info["bytes_received_per_frame"],
                            "gathered_image": "RGBA16F sky image (BHRAY_F_GATHER_SKY: every partition resolves the sky over its own rows, 8 B per pixel travel)" if main_kw.get("gather_sky") else "RGBA32F frame (travels packed - x, y, z + one bit of alpha, which is exactly 0 or 1: 12.1 B per pixel - and is unpacked by the root's de-interleave: the same bits)",
                            "batches_gathered": int(tm.gathers), "receive_ms_per_batch": round(tm.gather_ms / g, 5),
                            "deinterleave_ms_per_batch": round(tm.deinterleave_ms / g, 5),
                            "note": "receive = first ncclRecv enqueued -> all tiles of the batch arrived (includes waiting for the slowest partition's render); "
                                    "de-interleave = HIP kernel, staging rows -> frame rows, HBM-bound"}
            # N > 1: what the committed per-rank emulation (every rank of the partition rendered in turn on ONE GPU, before the gather: profiles/r04_emulate_*.json,
            # profiles/emulate_all_ranks.sh) says this command should scale like, and what the links allow - so that a hardware number can be read against both
            expected_d = None
            if n_gpus > 1:
                tagf = {(1920, 1080): "1080p", (3840, 2160): "4k", (7680, 4320): "8k"}.get((args.width, args.height))
                epath = os.path.join(ROOT, "profiles", f"r04_emulate_{tagf}.json") if tagf else ""
                emu = json.load(open(epath)) if epath and os.path.exists(epath) else {}
                short_, long_ = emu.get(f"{tagf}_n{n_gpus}_short", {}), emu.get(f"{tagf}_n{n_gpus}_long", {})
                per_link_mb = info["bytes_received_per_frame"] / max(1, n_gpus - 1) / 1e6
                link_gbs = 48.0
                # both gathers, whichever this run used: the rows the root receives x the bytes a row has on the wire
                wire_used_ = args.width * 8 if main_kw.get("gather_sky") else (3 * args.width + (args.width + 31) // 32) * 4
                rows_received_ = info["bytes_received_per_frame"] / float(wire_used_)
                n1_ms_ = (emu.get("n1_long", {}).get("ms_per_step") or ms_per_step * n_gpus)

                def links_for_(wire_row_bytes):
                    mb_ = rows_received_ * wire_row_bytes / max(1, n_gpus - 1) / 1e6
                    return {"mb_per_frame_and_link_into_the_root": round(mb_, 3), "ms_per_frame_on_the_links": round(mb_ / link_gbs, 5),
                            "link_bound_scaling": round(n1_ms_ / max(1e-9, mb_ / link_gbs), 2)}
                links_by_gather = {"rgba32f_packed": links_for_((3 * args.width + (args.width + 31) // 32) * 4), "rgba16f_sky": links_for_(args.width * 8),
                                   "used": "rgba16f_sky" if main_kw.get("gather_sky") else "rgba32f_packed",
                                   "why": ("--gather-sky: the RGBA16F image of the sky pass travels (BHRAY_F_GATHER_SKY: 8 bytes per pixel; the RGBA32F frame is never assembled)" if main_kw.get("gather_sky") else
                                           "the RGBA32F frame is gathered by default because that is what the metric names - north_star: `an RCCL gather over xGMI of the per-tile HDR buffer` of the RAY pass, "
                                           "the texture RayPipeline::output_view hands to the sky pass (ray_pipeline.rs:297-299) - although the root's links bound it earlier (link_bound_scaling); "
                                           "a host that only displays the frame gathers the sky pass's RGBA16F image instead: `--gather-sky`, half the bytes, the same pixels on screen (tests/test_gpu_multidevice.py)"),
                                   "assumed_gb_per_s_per_link_one_way": link_gbs, "n1_ms_per_frame": round(n1_ms_, 5)}
                expected_d = {"source": os.path.relpath(epath, ROOT) if emu else None,
                              "slowest_rank_scaling_in_blocks_of_%d_frames" % emu.get("n1_short", {}).get("steps", 20): short_.get("scaling"),
                              "slowest_rank_scaling_sustained": long_.get("scaling"),
                              "note": "compute only: the slowest rank's time per frame against the undivided frame on one GPU, emulated rank by rank; a block of exactly --steps frames is a chain "
                                      "of dependent ray generations per batch (chain-bound), a long block is throughput-bound",
                              "link_bound_scaling": links_by_gather,
                              "links": {"mb_per_frame_and_link_into_the_root": round(per_link_mb, 3), "assumed_gb_per_s_per_link_one_way": link_gbs,
                                        "ms_per_frame_on_the_links": round(per_link_mb / link_gbs, 5),
                                        "scaling_bound_by_the_links": round((emu.get("n1_long", {}).get("ms_per_step") or ms_per_step * n_gpus) / max(1e-9, per_link_mb / link_gbs), 2) if emu else None,
                                        "note": "every frame's tiles travel to the root over its %d links in parallel; the gather of a batch overlaps the next batch's render, so the links bound the SUSTAINED rate "
                                                "(and add the last batch's transfer to a short block).  48 GB/s one way per link is what RCCL send/recv typically sustains over xGMI - an assumption here, no "
                                                "multi-GPU node has measured it for this project yet; --gather-sky halves the bytes" % (n_gpus - 1)}}
            traced_rate = counters["traced"] * args.steps / elapsed / 1e6
            ref_host_regime = None
            try:
                leg_ = dropin["legs"]["async_sky_rgba16f_2_in_flight"]
                ref_host_regime = {"value": leg_["mrays_per_s"], "ms_per_frame": leg_["ms_per_frame"], "frames_in_flight": leg_["frames_in_flight"], "leg": "dropin.legs.async_sky_rgba16f_2_in_flight",
                                   "frame": dropin.get("frame"), "note": "bhusie_amd/bhray_render --dropin: update + pass + sky pass + hand-off per frame, PCIe-inclusive, without BHRAY_F_TEMPORAL"}
            except (TypeError, KeyError):
                pass
            # the compiler libbhray was (or would be) built with where the bench runs - the kernels' performance is a property of its schedule (VERDICT r5 weak 9;
            # __graft_entry__.build() refuses another major.minor, tests/test_gpu_perf_guard.py holds the numbers)
            try:
                import __graft_entry__ as ge_
                toolchain_d = dict(ge_.hipcc_version(), pinned_major_minor=ge_.PINNED_HIP)
            except Exception as e_:                  # never fail the bench line over the version string
                toolchain_d = {"error": f"{type(e_).__name__}: {e_}"}
        out = {
            "metric": "Mrays/sec at 1920x1080 adaptive-RK4; 1/2/4/8 MI355X + % HBM roofline",
            "value": round(value, 3), "unit": "Mrays/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic (seeded LUT and sky textures - color.png is an image asset, sky.png is missing from the reference checkout; disk texture = the reference's "
                    "disk.png regenerated by its own asset tool restated behind the ABI; default camera / hole / details of the reference" + (", time 0)" if args.static_time else ", time += 1/60 per frame as the reference's render loop, mod.rs:382)"),
            "value_definition": "final-level pixels of the frame x frames / time (BASELINE.md: pixels delivered by the adaptive pass; "
                                "82 % of them are copied or interpolated from the coarser ladder level, see traced_mrays_per_s), with "
                                f"frames_in_flight = {args.frames_in_flight} frames of the scene (the camera at rest, time advancing) enqueued ahead on as many HIP streams - which needs "
                                f"GPU_MAX_HW_QUEUES = {os.environ.get('GPU_MAX_HW_QUEUES')} exported before HIP initialises (bench.py does; ROCm's default of 4 "
                                "serialises the streams pairwise).  The reference host presents every frame (frame latency 2): its regimes are "
                                "latency_ms_one_frame_in_flight and `dropin`",
            "host_issue_ms_per_step": round(host_issue_ms, 5),
            "timed_blocks": {"blocks": len(blocks), "steps_per_block": args.steps, "reported": "median block" if len(blocks) > 1 else "the one block",
                             "block_ms": {"min": round(min(blocks) * 1e3, 4), "median": round(elapsed * 1e3, 4), "max": round(max(blocks) * 1e3, 4), "first": round(blocks[0] * 1e3, 4)},
                             "note": "every block = exactly --steps frames bracketed by barrier + full device synchronisation (pipeline fill and drain inside)"},
            "config": {
                "workload": ("configs[2]: " if args.workload == "mesh" else "configs[1]: ")
                + f"{args.width}x{args.height} " + ("adaptive RK (Cash-Karp)" if args.integrator == "rk" else "Euler") + ", accretion disk + adaptive background grid"
                + (f" + BVH mesh (327680-triangle icosphere OBJ, {args.bvh} builder) at (-10,0,30)" if args.workload == "mesh" else ""),
                "ladder": [list(s) for s in cfg.sizes()], "crop": [int(cfg.crop_x), int(cfg.crop_y)],
                "step_size": 0.15, "max_iterations": args.max_iterations, "angle_division_threshold": 0.02,
                "parallelism": (f"row-tiled x{n_gpus} ({partition_d['mode']}), in-library RCCL gather of every batch of {fpb} frames to partition {args.gather_root}'s GPU + HIP de-interleave")
                if n_gpus > 1 else "single GPU",
                "partition": partition_d,
                "frames_in_flight": args.frames_in_flight, "frames_per_batch": fpb, "gather_root": (args.gather_root if n_gpus > 1 else None),
                "verified_frames": verified, "speculative_levels": spec, "superset_levels": args.superset_levels, "readback_to_host": args.readback,
                "integrator_evaluation": args.eval, "emulated_rank": ([args.emulate_rank, args.emulate_world] if args.emulate_world else None),
            },
        }
        if args.full:
            out["config"].update({
                # (repeated here from the top level: the driver's `parsed` record keeps `config` whole and lists the other keys by name only)
                "mrays_per_s_reference_host_regime": ref_host_regime,
                "value_literal": literal_d["mrays_per_s"] if literal_d else None,
                "pixels_beyond_1e-4_vs_shader_text": ({k_: literal_d["distance_of_the_headline_kernel"][k_] for k_ in ("pixels_beyond_1e-4", "pixels", "fraction_beyond_1e-4", "class_differences", "max_rel_err")}
                                                      if literal_d else None),
                "toolchain": toolchain_d,
            })
            out.update({
                "traced_mrays_per_s": round(traced_rate, 3),
                "traced_fraction_of_frame_pixels": round(counters["traced"] / float(pixels), 4),
                "latency_ms_one_frame_in_flight": round(lat_ms, 4) if lat_ms else None,
                "latency_ms_one_frame_in_flight_by_mode": lat_modes,
                "mrays_per_s_one_frame_in_flight": round(pixels / (lat_ms * 1e-3) / 1e6, 2) if lat_ms else None,
                "sustained": sustained,
                "roofline": {
                    "bound": "hbm", "kernel": "trace_kernel", "achieved": round(achieved_gbs, 4), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved_gbs / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_note": traffic_note,
                    "avg_launch_ms": round(avg_ms, 5), "launches": exec_launches or int(tm.trace_launches),
                    "avg_launch_ms_definition": "execution span of the kernel (first block start -> last block end on the device clock, stamped by the kernel: bhray_timing.trace_exec_ms); "
                                                "agrees with rocprofv3 --kernel-trace --stats of this command (profiles/)" if exec_launches else "HIP events around the launch (no execution spans recorded)",
                    "avg_launch_ms_enqueue_to_complete": round(enq_ms, 5),
                    "algorithmic_bytes_per_launch": round(bytes_per_launch, 1),
                    "concurrency": f"{args.frames_in_flight} frames in flight: a launch shares the device with the kernels it overlaps with; spans and events are taken on "
                                   "every 4th batch of the timed region (every event is a packet in the stream: all of them cost 1.6 %)",
                    "isolated": iso_d,
                    "frac_from_profiles": frac_from_profiles,
                    "secondary": {"bound": "valu", "achieved": round(valu_tflops, 4), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": round(valu_tflops / VALU_PEAK_TFLOPS, 6)},
                    "note": "the metric names the HBM roofline, so `bound`/`frac` are HBM; the kernel is a VALU-bound f32 ODE march (SURVEY.md F8: ~20 "
                            "algorithmic bytes per traced ray against ~96 kflop), so the fraction that says something about the kernel is `secondary` (= `valu`)",
                },
                "valu": {"achieved": round(valu_tflops, 4), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(valu_tflops / VALU_PEAK_TFLOPS, 6),
                         "algorithmic_flops_per_frame": flops_per_frame,
                         "one_frame_in_flight": ({"achieved": round(flops_per_frame / (lat_ms * 1e-3) / 1e12, 4), "frac": round(flops_per_frame / (lat_ms * 1e-3) / 1e12 / VALU_PEAK_TFLOPS, 6),
                                                  "note": "the same flops / latency_ms_one_frame_in_flight: the reference host's regime, where every launch lasts as long as its longest ray"}
                                                 if lat_ms else None),
                         "issue": valu_issue,
                         "note": "algorithmic flops per frame (390 per RK step as the shader text counts them; the kernel issues fewer operations since N9/N10) / "
                                 "wall time per frame of the median block; peak = the FMA rate"},
                "pass_ms": {"event_total": round(tm.total_ms / frames, 5), "trace": round(tm.trace_ms / frames, 5),
                            "classify": round(tm.classify_ms / frames, 5),
                            "level_trace": [round(tm.level_trace_ms[i] / frames, 5) for i in range(args.levels)]},
                "gather": gather_d,
                "expected_scaling": expected_d,
                # the reference host's regime as a second headline: the C++ mirror of the Rust shim - one host thread, the shipped 72x41 x3 x4
                # ladder, two frames in flight (mod.rs:108 desired_maximum_frame_latency: 2), every frame through the sky pass and handed to pinned host memory as
                # RGBA16F, NO temporal history - from the `dropin` leg of this run
                "mrays_per_s_reference_host_regime": ref_host_regime,
                "value_literal": literal_d["mrays_per_s"] if literal_d else None,
                "value_literal_definition": ("the same timed blocks rendered by the LITERAL kernel (BHRAY_F_LITERAL: ray.wgsl:401-480 operator by operator, bit-identical to the "
                                             "executed shader text on every direction pixel): the number that meets north_star's 1e-4 per channel to the letter; `value` is the contract "
                                             "evaluation (FMA + reassociation, DESIGN.md N7/N9/N10)") if literal_d else None,
                "pixels_beyond_1e-4_vs_shader_text": literal_d["distance_of_the_headline_kernel"] if literal_d else None,
                "literal": literal_d,
                "handoff": handoff_d,
                "dropin": dropin,
                "sequence": sequence_d,
                "mrays_per_s_with_handoff": handoff_d["mrays_per_s_with_handoff"] if handoff_d else None,
                "sky_resolve": sky_d,
                "counters": counters,
                "algorithmic_bytes_per_frame": algorithmic_bytes_frame(counters),
            })
        if n_gpus == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, tex, cam, bh, det, model)
        print(json.dumps(out), flush=True)
    if rp is not None:
        rp.close()
    launcher.close()


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except Exception as e:                       # one line on stderr and a non-zero exit code: a bhray / RCCL error text, not a Python traceback, is what the driver's log should show
        import traceback
        print(f"bench: FAILED on rank {os.environ.get('RANK', '0')}: {type(e).__name__}: {e}", file=sys.stderr)
        traceback.print_exc(file=sys.stderr)
        sys.exit(2)
