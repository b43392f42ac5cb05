"""CPU: bhray_trace_grid_for (bhusie_amd/csrc/bhray_layout.cpp, include/bhray_diag.h) - the persistent grid a dense ladder trace launch gets from the rays its queues
held the last time: blocks = ceil(expected * (100 + margin) / 100 / rays per block generation), clamped to [max(frames in the batch, floor), ctx grid].  Pure host
arithmetic: no device is touched."""
import ctypes as C

import bhusie_amd as B
from bhusie_amd import layouts

NONE = layouts.LEVEL_GRID_NO_FEEDBACK
GEN, MARGIN, FLOOR = 256, 25, 64          # the defaults (BHRAY_LEVEL_GRID_GEN / _MARGIN / _FLOOR)


def grid_for(expected, frames=1, ctx_grid=512, gen=GEN, margin=MARGIN, floor=FLOOR):
    return int(B.lib().bhray_trace_grid_for(expected, frames, ctx_grid, gen, margin, floor))


def test_the_formula():
    # 1 000 rays + 25 % = 1 250 rays = 4.88 blocks of 256
    assert grid_for(1000, floor=0) == 5
    assert grid_for(1024, margin=0, floor=0) == 4 and grid_for(1025, margin=0, floor=0) == 5
    assert grid_for(1024, margin=0, floor=0, gen=512) == 2
    # the coarse launches of the 1920x1080 ladder: about 27 k and 40 k rays in a 512-block grid
    assert grid_for(27000) == 132 and grid_for(40000) == 196


def test_clamp_to_the_batch_size_the_floor_and_the_ceiling():
    for frames in (1, 3, 32):
        assert grid_for(1, frames=frames, floor=0) == frames          # every frame of a batch needs a block that starts with it
        assert grid_for(1, frames=frames, floor=8) == max(frames, 8)
    assert grid_for(10 ** 6) == 512 and grid_for(10 ** 6, ctx_grid=384) == 384
    # the ceiling wins over the floor and over the batch size: no launch gets a larger grid than the ctx's
    assert grid_for(100, frames=40, ctx_grid=32) == 32 and grid_for(100, ctx_grid=16, floor=64) == 16


def test_zero_expected_rays():
    assert grid_for(0, floor=0) == 1 and grid_for(0, frames=3, floor=0) == 3 and grid_for(0) == FLOOR and grid_for(0, frames=3, margin=0, floor=2) == 3


def test_without_feedback_the_launch_gets_the_ctx_grid():
    for ctx_grid in (1, 384, 512, 1024):
        assert grid_for(NONE, ctx_grid=ctx_grid) == ctx_grid
        assert grid_for(NONE, frames=5, ctx_grid=ctx_grid, floor=0) == ctx_grid
    assert grid_for(1000, gen=0) == 512                                # (a generation of no rays sizes nothing)


def test_monotone_in_the_expected_rays():
    for frames, ctx_grid, gen, margin, floor in ((1, 512, 256, 25, 64), (3, 384, 512, 0, 0), (8, 1024, 256, 100, 16)):
        prev = 0
        for e in sorted(set(list(range(0, 4000, 7)) + [min(2 ** k + d, 2 ** 32 - 1) for k in range(10, 33) for d in (-1, 0, 1)])):
            g = grid_for(e, frames, ctx_grid, gen, margin, floor)
            assert min(max(frames, floor), ctx_grid) <= g <= ctx_grid
            assert g >= prev, (e, g, prev)
            prev = g


def want(expected, gen=GEN, margin=MARGIN):
    """the formula in Python's unbounded integers"""
    return -(-(-(-expected * (100 + margin) // 100)) // gen)


def test_no_overflow_at_the_largest_queue():
    big, wide = 2 ** 32 - 1, 2 ** 32 - 1
    assert grid_for(big) == 512
    assert want(big) == 20971520 and grid_for(big, ctx_grid=wide, floor=0) == want(big)                 # nothing wrapped
    assert grid_for(32 * big, frames=32, ctx_grid=wide, gen=4096, margin=1000, floor=0) == want(32 * big, gen=4096, margin=1000)    # a batch of 32 such queues, the largest margin
    assert grid_for(big, ctx_grid=wide, margin=2 ** 32 - 1, floor=0) == want(big, margin=1000)           # the margin is capped at 1000 %


def test_the_defaults_reproduce_the_ctx_grid_for_a_full_queue():
    """One generation of 256 rays per block: a queue of at least ctx_grid * 256 rays gets the ctx's grid - the last level of a saturated ladder is launched as before."""
    for ctx_grid in (384, 512, 1024):
        for extra in (0, 1, 1000, 10 ** 6):
            assert grid_for(ctx_grid * 256 + extra, ctx_grid=ctx_grid) == ctx_grid
    assert grid_for(298920) == 512                                     # the 1920x1080 ladder's last level


def test_the_struct_the_getter_fills():
    g = layouts.BhrayLevelGridInfo()
    assert C.sizeof(g) == 12 * (layouts.MAX_LEVELS + 2) + 40 and layouts.BhrayLevelGridInfo.blocks.offset == 8 * (layouts.MAX_LEVELS + 2) + 24
    assert g.as_dict()["launches"] == {}
