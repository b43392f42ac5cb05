"""-m gpu: trace grids sized by queue length (launch_batch in bhusie_amd/csrc/bhray_api.hip, bhray_trace_grid_for).  A dense ladder trace launch gets
enough persistent blocks for the rays its queues held the last time its slot position ran, not the ctx's grid.  Scheduling only: every case renders the same frames with
the rule on and with BHRAY_LEVEL_GRID=0 (read at create) in the same library and compares them with bench.py's rule - bit for bit, the sign of a NaN excepted -, and reads
WHAT the rule did from bhray_get_level_grids, not from a clock.  The dense builds are forced with BHRAY_TRACE_DENSE=1 (read at create), not by a 1080p frame."""
import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import layouts
from tests import common as T

pytestmark = pytest.mark.gpu

GEN, MARGIN, FLOOR = 256, 25, 64                                     # the rule's defaults
SUPERSET = layouts.MAX_LEVELS + 1                                    # launch ids of bhray_level_grid_info: 0 the speculative launch, 1 + l level l, this the superset launch
OFF = (1.5, -0.75, 2.0)
OUTSIDE = dict(position=(0.0, 3.0, -45.0), forward=(0.0, -3.0 / 45.1, 45.0 / 45.1), fov=1.0)      # a camera outside the sphere, the hole in view
AWAY = dict(position=(0.0, 0.0, -19.0), forward=(0.0, 0.0, -1.0), fov=1.0)                          # the default camera turned away from the hole: nothing but sky
# Rays traced per level, counted by the CPU oracle (oracle.render_level's counters; RK).  Looking AWAY with a wide threshold all but a few border pixels interpolate:
#   96x54 x3 levels:  AWAY, threshold 4.0: 84, 8, 36 (the 36 in the level's margin around the frame: the last level's queue, which holds the frame's crop only, is empty)
#   160x90 x4 levels: AWAY, threshold 0.5: 35, 16, 36, 82;   the default camera, threshold 0.5: 35, 116, 496, 3460
# (a camera outside the relativity sphere traces every pixel of every level at these sizes, whatever it looks at)


def small():
    return B.ladder_for_frame((96, 54), 3, 3)


def four():
    return B.ladder_for_frame((160, 90), 3, 4)


def differing_pixels(a, b):
    """bench.py's rule: bit for bit, except the sign of a NaN both frames have"""
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    wa, wb = a.view(np.uint32).copy(), b.view(np.uint32).copy()
    wa[na & nb] = 0
    wb[na & nb] = 0
    return int((wa != wb).any(axis=-1).sum())


def same_frames(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        n = differing_pixels(x, y)
        assert n == 0, f"{what}, frame {i}: {n} pixels differ between the sized grids and BHRAY_LEVEL_GRID=0"


def grid_for(expected, frames, ctx_grid, floor=FLOOR):
    return int(B.lib().bhray_trace_grid_for(expected, frames, ctx_grid, GEN, MARGIN, floor))


def run(cfg, seq, kw, tex, model=None, every_frame=True, lensing=False):
    """Renders the frames of seq; returns (frames read, the getter's record of every batch in launch order).  every_frame: each frame is waited for and read before the
    next is staged, so a slot position's feedback is its previous use; otherwise the frames are enqueued ahead as bench.py does and only the last is read."""
    rp = B.RayPass(cfg, device=0, **kw)
    rp.set_textures(*tex)
    if model is not None:
        rp.upload_model(model)
    if lensing:
        rp.set_mesh_lensing(True)
    fpb, slots = max(1, kw.get("frames_per_batch", 0)), kw.get("frames_in_flight", 0) or 4
    frames, grids = [], []
    for i, u in enumerate(seq):
        rp.set_uniforms(*u)
        rp.render()
        if (i + 1) % fpb == 0:
            if every_frame:
                rp.sync()
                if rp.read_hdr().size:
                    frames.append(rp.read_hdr().copy())
            grids.append(rp.level_grids(((i + 1) // fpb - 1) % slots))
    rp.sync()
    if not every_frame:
        frames.append(rp.read_hdr().copy())
    rp.close()
    return frames, grids


def on_and_off(monkeypatch, fn):
    monkeypatch.setenv("BHRAY_TRACE_DENSE", "1")
    monkeypatch.setenv("BHRAY_LEVEL_GRID", "1")
    a = fn()
    monkeypatch.setenv("BHRAY_LEVEL_GRID", "0")
    b = fn()
    monkeypatch.delenv("BHRAY_LEVEL_GRID", raising=False)
    return a, b


def check_rule(grids, slots, frames_per_batch=1, floor=FLOOR, what=""):
    """The first use of every slot position gets the ctx's grid; every later one is sized from what the getter says it expected, by the rule, within the clamp."""
    shrunk = 0
    for n, g in enumerate(grids):
        assert g["enabled"] and g["dense"] and g["frames"] == frames_per_batch and g["launches"], (what, n, g)
        for lid, (blocks, expected) in g["launches"].items():
            if n < slots:
                assert expected is None and blocks == g["ctx_grid"], f"{what}: batch {n} is the first use of its slot, launch {lid}: {blocks} blocks from {expected} rays"
            else:
                assert expected is not None, f"{what}: batch {n}, launch {lid}: no feedback although its slot has run before"
                assert blocks == grid_for(expected, frames_per_batch, g["ctx_grid"], floor), (what, n, lid, blocks, expected)
                assert min(max(frames_per_batch, floor), g["ctx_grid"]) <= blocks <= g["ctx_grid"], (what, n, lid, blocks)
                shrunk += blocks < g["ctx_grid"]
    assert shrunk > 0, f"{what}: no grid shrank after the first round: {grids[-1]}"


def check_off(grids, what=""):
    for n, g in enumerate(grids):
        assert not g["enabled"]
        for lid, (blocks, expected) in g["launches"].items():
            assert expected is None and blocks == g["ctx_grid"], f"{what}: BHRAY_LEVEL_GRID=0, batch {n}, launch {lid}: {blocks} blocks of {g['ctx_grid']}"


@pytest.mark.parametrize("method", [0, 1])
def test_eight_slots_the_grids_shrink_after_the_first_round(monkeypatch, method):
    """RK and Euler, 8 frame slots, 26 frames of the bench's loop (time advancing): every slot position is used three times."""
    tex = T.textures()
    seq = [T.uniforms(integration_method=method, time=k / 60.0) for k in range(26)]
    for cfg, kw in ((small(), dict(frames_in_flight=8, speculative_levels=2)), (four(), dict(frames_in_flight=8))):
        (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(cfg, seq, kw, tex))
        same_frames(a, b, f"8 slots, method {method}, {kw}")
        check_rule(ga, 8, what=f"method {method}, {kw}")
        check_off(gb)
        print(f"method {method} {kw}: ctx grid {ga[-1]['ctx_grid']}, last batch {ga[-1]['launches']}, blocks {ga[-1]['total_blocks']} in {ga[-1]['total_launches']} launches "
              f"({ga[-1]['total_ceiling_launches']} at the ceiling) against {gb[-1]['total_blocks']}")
        assert ga[-1]["total_launches"] == gb[-1]["total_launches"] and ga[-1]["total_blocks"] < gb[-1]["total_blocks"]
        assert gb[-1]["total_ceiling_launches"] == gb[-1]["total_launches"]


def test_batches_of_three_with_an_empty_queue(monkeypatch):
    """frames_per_batch = 3, no floor but the batch's own: a frame that looks away from the hole with a wide threshold queues 8 rays for level 1 and none for the last level
    (the level's few traced border pixels lie outside the frame's crop), so a launch sized from 0 rays gets one block per frame of the batch and never fewer."""
    monkeypatch.setenv("BHRAY_LEVEL_GRID_FLOOR", "0")
    tex = T.textures()
    hole = T.uniforms(integration_method=1, camera=B.Camera(**OUTSIDE))
    empty = T.uniforms(integration_method=1, camera=B.Camera(**AWAY), angle_division_threshold=4.0)
    seq = ([empty] * 3 + [hole, empty, hole]) * 3                                  # slot 0: three frames of sky; slot 1: a nearly empty queue between two others
    kw = dict(frames_in_flight=2, frames_per_batch=3)
    (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(small(), seq, kw, tex))
    same_frames(a, b, "batches of three")
    check_rule(ga, 2, frames_per_batch=3, floor=0, what="batches of three")
    check_off(gb)
    sized = [(blocks, expected) for g in ga[2:] for blocks, expected in g["launches"].values()]
    print("batches of three:", [g["launches"] for g in ga])
    assert all(blocks >= 3 for blocks, _ in sized)
    assert any(expected == 3 * 8 and blocks == 3 for blocks, expected in sized) and any(expected == 0 and blocks == 3 for blocks, expected in sized), \
        f"no launch was sized from three empty queues: {sized}"
    mixed = [g["launches"][3] + (g["ctx_grid"],) for g in ga[3::2]]                # slot 1, the last level: two frames with the hole and one that reported 0 rays
    assert all(expected > 0 and blocks == grid_for(expected, 3, ctx_grid, 0) for blocks, expected, ctx_grid in mixed), mixed


@pytest.mark.parametrize("kw,ids", [(dict(speculative_levels=0), {1, 2, 3, 4}), (dict(speculative_levels=2), {0, 3, 4}),
                                    (dict(superset_levels=2), {1, 2, SUPERSET}), (dict(speculative_levels=2, superset_levels=2), {0, SUPERSET})])
def test_speculative_and_superset_launches(monkeypatch, kw, ids):
    """The merged launch of the speculative levels, the plain levels and the superset launch each keep a word of their own.  (superset_levels is 0 or 2..4: bhray_create
    refuses 1, so the superset cases trace the last two levels in one launch.)"""
    tex = T.textures()
    seq = [T.uniforms(integration_method=1, time=k / 60.0) for k in range(9)]
    kw = dict(frames_in_flight=3, **kw)
    (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(four(), seq, kw, tex))
    same_frames(a, b, f"{kw}")
    check_rule(ga, 3, what=f"{kw}")
    check_off(gb)
    assert all(set(g["launches"]) == ids for g in ga), (ids, ga[-1]["launches"])


@pytest.mark.parametrize("method", [0, 1])
def test_mesh_variant(monkeypatch, tmp_path, method):
    from bhusie_amd import assets
    tex = T.textures()
    p = tmp_path / "mesh.obj"
    p.write_text(assets.icosphere_mesh_obj(2, radius=6.0, bump=0.2, seed=11))
    model = B.load_model(str(p))
    model.set_transform((-7.0, 1.0, 24.0), 1)
    seq = [T.uniforms(integration_method=method, model_count=1, time=k / 60.0) for k in range(7)]
    kw = dict(frames_in_flight=3, speculative_levels=2)
    (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(small(), seq, kw, tex, model=model))
    same_frames(a, b, f"mesh, method {method}")
    check_rule(ga, 3, what=f"mesh, method {method}")
    check_off(gb)


@pytest.mark.parametrize("case", ["lensed", "literal", "eval_fma"])
def test_mesh_launches_that_get_the_latency_build_keep_their_grids(monkeypatch, tmp_path, case):
    """A lensed-mesh ctx, and the mesh variant under the literal / fma evaluations, have no dense build: a launch that asks for one runs the latency build, whose thin
    shares are dealt by gridDim.  The getter must say so (dense 0) and every launch, on every use of a slot, must keep the ctx's grid."""
    from bhusie_amd import assets
    tex = T.textures()
    p = tmp_path / "mesh.obj"
    p.write_text(assets.icosphere_mesh_obj(2, radius=6.0, bump=0.2, seed=11))
    model = B.load_model(str(p))
    model.set_transform((4.0, 0.0, -8.0) if case == "lensed" else (-7.0, 1.0, 24.0), 1)
    seq = [T.uniforms(integration_method=1, model_count=1, time=k / 60.0) for k in range(7)]
    kw = dict(frames_in_flight=3, speculative_levels=2, **({} if case == "lensed" else {case: True}))
    (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(small(), seq, kw, tex, model=model, lensing=case == "lensed"))
    same_frames(a, b, case)
    assert [g["launches"] for g in ga] == [g["launches"] for g in gb], f"{case}: the grids moved"
    for g in ga + gb:
        assert not g["dense"] and g["launches"], (case, g)
        assert all(blocks == g["ctx_grid"] and expected is None for blocks, expected in g["launches"].values()), (case, g)
    assert all(g["enabled"] for g in ga) and ga[-1]["total_ceiling_launches"] == ga[-1]["total_launches"]


def test_ranks_of_a_row_partition(monkeypatch):
    """Both ranks of a 2-way striped partition, a slab, and a rank that owns no rows: it launches nothing and the getter says so."""
    tex = T.textures()
    seq = [T.uniforms(integration_method=1, time=k / 60.0) for k in range(7)]
    for part in (dict(row_rank=0, row_world=2, stripe_rows=9), dict(row_rank=1, row_world=2, stripe_rows=9), dict(row_rank=1, row_world=2, slab_row0=[0, 30, 54])):
        kw = dict(frames_in_flight=3, speculative_levels=2, **part)
        (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(small(), seq, kw, tex))
        same_frames(a, b, f"{part}")
        check_rule(ga, 3, what=f"{part}")
        check_off(gb)
    kw = dict(frames_in_flight=3, speculative_levels=2, row_rank=1, row_world=2, slab_row0=[0, 54, 54])
    (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(small(), seq, kw, tex))
    assert a == [] and b == []
    assert all(g["launches"] == {} and g["total_launches"] == 0 for g in ga + gb)


def test_scene_cut(monkeypatch):
    """The camera turns from empty sky to the hole between two uses of a slot position: the launches of the first frame with the hole are sized for next to nothing (no
    floor here), find a queue more than ten times that - the same slot's next use reports it - and render the same frame, only later."""
    monkeypatch.setenv("BHRAY_LEVEL_GRID_FLOOR", "0")
    tex = T.textures()
    sky, hole = T.uniforms(integration_method=1, camera=B.Camera(**AWAY), angle_division_threshold=0.5), T.uniforms(integration_method=1, angle_division_threshold=0.5)
    seq = [sky] * 4 + [hole] * 4
    kw = dict(frames_in_flight=2)
    (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(four(), seq, kw, tex))
    same_frames(a, b, "scene cut")
    check_off(gb)
    undersized = 0
    for n in (4, 5):                                                 # the first frame with the hole, in either slot: sized from a frame of sky
        cut, after = ga[n]["launches"], ga[n + 2]["launches"]        # ... and the slot's next use, sized from what the cut frame's queues really held
        print(f"scene cut, batch {n}: (blocks, expected rays) {cut}; the queues held {({k: v[1] for k, v in after.items()})}")
        for lid, (blocks, expected) in cut.items():
            held = after[lid][1]
            assert expected is not None and held is not None
            if held > 10 * max(expected, 1) and blocks * GEN < held:
                undersized += 1
    assert undersized >= 2, "the cut did not leave a launch with a grid too small for its queue: the scene of this test is wrong"


@pytest.mark.parametrize("method", [0, 1])
def test_moving_time_and_a_hole_that_leaves_the_origin(monkeypatch, method):
    """The bench's own loop - frames enqueued ahead, nothing waited for - with the hole off the origin and back: the build and the grid change per launch.  Enqueued ahead,
    a slot's feedback is its previous use or the one before (whichever has reported), so only the clamp is asserted here, and the last frame's bytes."""
    tex = T.textures()
    pos = [(0.0, 0.0, 0.0), OFF, (0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.25, 0.0, 0.0)] * 3
    seq = [T.uniforms(integration_method=method, black_hole=B.BlackHole(position=p), time=k / 60.0) for k, p in enumerate(pos)]
    for cfg, kw in ((small(), dict(frames_in_flight=3, speculative_levels=2)), (four(), dict(frames_in_flight=4))):
        (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(cfg, seq, kw, tex, every_frame=False))
        same_frames(a, b, f"moving hole, enqueued ahead, method {method}, {kw}")
        (a, ga2), (b, _) = on_and_off(monkeypatch, lambda: run(cfg, seq, kw, tex))
        same_frames(a, b, f"moving hole, method {method}, {kw}")
        check_rule(ga2, kw["frames_in_flight"], what=f"moving hole, method {method}")
        for g in ga:
            for blocks, expected in g["launches"].values():
                assert (blocks == g["ctx_grid"]) if expected is None else (blocks == grid_for(expected, 1, g["ctx_grid"]))
        check_off(gb)


def test_counting_and_temporal_ctxs_keep_their_grids(monkeypatch):
    """A counting ctx and a BHRAY_F_TEMPORAL ctx are left alone: the getter reports the same grids with the rule on and off, none of them sized."""
    tex = T.textures()
    seq = [T.uniforms(integration_method=1, time=k / 60.0) for k in range(5)]
    for kw in (dict(frames_in_flight=2, counters=True, speculative_levels=2), dict(frames_in_flight=2, temporal=True), dict(frames_in_flight=1, temporal=True)):
        (a, ga), (b, gb) = on_and_off(monkeypatch, lambda: run(small(), seq, kw, tex))
        same_frames(a, b, f"{kw}")
        assert [g["launches"] for g in ga] == [g["launches"] for g in gb], f"{kw}: the grids moved"
        for g in ga + gb:
            assert not g["enabled"] and g["launches"]
            assert all(expected is None for _, expected in g["launches"].values())
        assert ga[-1]["total_blocks"] == gb[-1]["total_blocks"]
