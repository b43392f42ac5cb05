"""CPU: the NumPy restatement of the ray paths (tests/ray_paths_ref.py) is tests/ray_records_ref.py's trace with bookkeeping added and nothing else
changed - its results, records and margins are that file's in every bit -, and its points are the ray: the counts follow the iterations, the end point is where the
record says, consecutive points inside the sphere are a step apart, and no point comes closer to the hole than the record's closest approach."""
import numpy as np
import pytest

import bhusie_amd as B
from tests import ray_paths_ref as PR
from tests import ray_records_ref as R
from tests import rays_ref as RR

REL = 1e-5                      # binary32 arithmetic on coordinates of a few tens: a step's length and a distance are good to a few ulp, 1e-5 relative is ~80 of them


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same_trace(got, want):
    out, rec, margin, after = got[:4]
    assert np.array_equal(_bits(out), _bits(want[0])), "results"
    assert rec.tobytes() == want[1].tobytes(), "records"
    assert np.array_equal(_bits(margin), _bits(want[2])), "margins"
    assert np.array_equal(after, want[3])


def _assert_counts_and_ends(rec, paths, counts):
    assert len(paths) == rec.shape[0] and [p.shape[0] for p in paths] == counts.tolist()
    for s in (0, 3, 16):
        want = (rec["iterations"] >> np.uint32(s)) + 2
        assert np.array_equal(PR.counts(rec, s), want)
        assert [PR.sample(p, s).shape[0] for p in paths] == want.tolist(), f"counts == (iterations >> {s}) + 2"
    for r, p in enumerate(paths):
        assert p.dtype == B.PATH_POINT_DTYPE and p["iteration"][0] == 0 and p["iteration"][-1] == rec["iterations"][r]
        assert np.array_equal(p["iteration"][:-1], np.arange(p.shape[0] - 1)), "one point per counted iteration"
        if (rec["hit"][r] & 0xFF) == B.HIT_NONE:
            assert np.array_equal(_bits(p["position"][-1]), _bits(rec["position"][r])), "a ray that hit nothing ends where its record says"


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_seeded_list(method):
    rays = RR.seeded_rays()[:PR.N_SEEDED]
    got = PR.seeded_reference(method)
    _assert_same_trace(got, R.trace(RR.scene_uniforms(method), rays))
    out, rec, margin, _, paths, counts = got
    assert int(rec["iterations"].max()) == (328, 811)[method] and int(counts.max()) <= PR.MAX_POINTS, "the GPU tests' rows of 1 024 points drop nothing"
    assert int((margin < R.MARGIN_BAR).sum()) == (0, 1)[method] <= R.MARGIN_SHARE * rays.shape[0]
    assert all(np.array_equal(_bits(p["position"][0]), _bits(rays[r, 0:3])) for r, p in enumerate(paths)), "point 0 is the origin"
    _assert_counts_and_ends(rec, paths, counts)
    k = R.kinds(rec)
    assert min(k["none"], k["horizon"], k["disk"]) >= 50, k


def test_the_mesh_list():
    got = PR.mesh_reference(1)
    _assert_same_trace(got, R.mesh_reference(1))
    out, rec, margin, _, paths, counts = got
    assert int(counts.max()) <= PR.MAX_POINTS and int((margin < R.MARGIN_BAR).sum()) <= R.MARGIN_SHARE * rec.shape[0]
    _assert_counts_and_ends(rec, paths, counts)
    mesh = np.nonzero((rec["hit"] & 0xFF) == B.HIT_MESH)[0]
    assert mesh.size >= 300
    for r in mesh:                                                # opacity 1: the hit ends the ray, where the record says
        assert np.array_equal(_bits(paths[r]["position"][-1]), _bits(rec["position"][r]))


def test_the_points_are_the_ray():
    """Euler, stride 1: two sanity checks that the points are the curve the integrator walked.

    The closest approach is the minimum over the INTEGRATOR's positions (ray.wgsl:533), and a hit moves curr.position from there by prev.direction * t, t < the step
    (ray.wgsl:571) - forwards, so a hit's point may lie nearer the hole than `closest` by up to one step.  Of these 1 027 rays 284 (211 horizon, 73 disk) have such a point,
    the largest shortfall being 0.139 of a step of 0.15.  So: every point of a ray that hit nothing, and every point in front of a ray's first hit, is no nearer than
    `closest` (1e-5 relative); every point whatsoever is no nearer than `closest` minus one step."""
    S = R.np_scene(RR.scene_uniforms(0))
    out, rec, margin, _, paths, counts = PR.seeded_reference(0)
    hole = np.asarray(S.bh_pos, dtype=np.float64)
    step, radius = float(S.step_size), float(S.R)
    steps = bounded = 0
    for r, p in enumerate(paths):
        pos = p["position"].astype(np.float64)
        dist = np.sqrt(((pos - hole) ** 2).sum(axis=1))
        closest = float(rec["closest"][r])
        # the first hit's point: where the record says (every point from there on may be a hit's)
        first = pos.shape[0]
        if (rec["hit"][r] & 0xFF) != B.HIT_NONE:
            same = np.nonzero((p["position"] == rec["position"][r]).all(axis=1))[0]
            assert same.size >= 1, f"ray {r}: its first hit's position is not among its points"
            first = int(same[0])
        assert dist[:first].min(initial=np.inf) >= closest * (1.0 - REL), (r, dist[:first].min(), closest)
        assert dist.min() >= closest - step * (1.0 + REL), (r, dist.min(), closest)
        bounded += int(dist.min() < closest * (1.0 - REL))
        # consecutive points with consecutive iterations, both inside the sphere, in front of the first hit: a step apart (an entry starts on the sphere's surface, an exit
        # ends outside it; a hit moves the point along the segment)
        body = min(first, pos.shape[0] - 1)
        d = np.sqrt(((pos[1:body] - pos[:body - 1]) ** 2).sum(axis=1)) if body >= 2 else np.zeros(0)
        ok = (dist[:body - 1] < radius * (1.0 - 1e-3)) & (dist[1:body] < radius * (1.0 - 1e-3)) if body >= 2 else np.zeros(0, bool)
        assert (np.abs(d[ok] - step) <= REL * step).all(), (r, d[ok][np.abs(d[ok] - step) > REL * step][:3], step)
        steps += int(ok.sum())
    print(f"{steps} steps inside the sphere compared; {bounded} rays have a hit's point nearer the hole than their closest approach")
    assert steps >= 20000, steps
