"""CPU: the NumPy reference of lensed ray batches and records (tests/lensed_rays_ref.py) against the two restatements it was put together from.

  1. On rays(259), both integrators: the results are tests/lensed_ref.py::trace_rays_lensed's in every bit, and the list shows what it is meant to show - the floors
     below, on the reference's own counts (RK / Euler here: segments a model won 57 / 71; first hit a mesh by a segment 42 / 58, per visible slot 12, 18, 12 / 17, 25, 16,
     naming the invisible slot 0 / 0; a model winning after a disk hit 15 / 13; first hit horizon, disk, none 21, 101, 69 / 26, 98, 72; margin rays 1 / 0; results that
     differ from the flat-space trace 52 / 70).
  2. Where no segment can meet a model - every model invisible; one mesh wholly beyond R + 5 - every result and record word is tests/ray_records_ref.py::trace's."""
import numpy as np
import pytest

from tests import lensed_ref as LR
from tests import lensed_rays_ref as LRR
from tests import ray_records_ref as RRR

N = LRR.N_RAYS_CPU


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rec_words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)


@pytest.mark.parametrize("method", [1, 0], ids=["rk", "euler"])
def test_results_are_lensed_refs_and_the_list_holds_its_floors(method):
    out, rec, margin, seg_first, st = LRR.reference(method, N)
    rays = LRR.rays(N)
    S = RRR.np_scene(LRR.uniforms(method), [m.arrays() for m in LRR.models()])
    stats = {}
    plain = LR.trace_rays_lensed(S, rays[:, 0:3].copy(), rays[:, 4:7].copy(), stats)
    assert np.array_equal(_bits(out), _bits(plain)), "the results are not lensed_ref.trace_rays_lensed's"
    assert stats["segment_hits"] == st["segment_hits"]
    c = LRR.conditions(method, N)
    print("method", method, c)
    LRR.assert_conditions(c, N)
    assert (_rec_words(rec)[:, 3] >> 16 == 0).all(), "bits 16-31 of `hit` are zero"
    tri = rec["triangle"][(rec["hit"] & 0xFF) == LRR.HIT_MESH]
    assert ((tri >= 0) & (tri < 80)).all() and (rec["triangle"][(rec["hit"] & 0xFF) != LRR.HIT_MESH] == -1).all()


@pytest.mark.parametrize("case", ["all_invisible", "one_mesh_beyond_R_plus_5"])
def test_without_a_model_in_reach_the_words_are_the_flat_space_records(case):
    if case == "all_invisible":
        slots, method = [(r, p, 0) for r, p, _ in LRR.SLOTS], 1
    else:       # one visible mesh, every point of it more than 25 from the hole (R = 20): no segment inside the sphere reaches it; rays still hit it in flat space
        slots, method = [(3, (3.5, -1.5, -8.0), 0), (4, (0.0, 6.0, 0.0), 0), (16, (0.5, 2.0, 44.0), 1), (8, (-10.0, 0.0, 17.0), 0)], 0
        far = LRR.model(*slots[2]).arrays()
        reach = np.linalg.norm(far["points"][:, :3].astype(np.float64) + np.asarray(slots[2][1]), axis=1).min()
        assert reach > 25.0, reach
    rays = LRR.rays(N)
    out, rec, margin, seg_first, st = LRR.trace(method, rays, slots)
    flat_out, flat_rec, flat_margin, _ = RRR.trace(LRR.uniforms(method), rays, [m.arrays() for m in LRR.models(slots)])
    assert st["segment_hits"] == 0 and not seg_first.any()
    assert np.array_equal(_bits(out), _bits(flat_out))
    assert np.array_equal(_rec_words(rec), _rec_words(flat_rec))
    assert np.array_equal(_bits(margin), _bits(flat_margin))
    if case != "all_invisible":
        assert int(((rec["hit"] & 0xFF) == LRR.HIT_MESH).sum()) >= 1, "the mesh beyond the sphere must be in the list's flat-space hits"
