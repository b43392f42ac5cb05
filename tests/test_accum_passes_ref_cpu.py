"""CPU: the still passes' per-sample rule - bhray_accum_pass_values, host arithmetic through the function the kernels call, against the NumPy
restatement tests/accum_passes_ref.py in every word, on a synthetic table that holds every branch of the rule; and the restatement's own sum and mean."""
import itertools

import numpy as np

import bhusie_amd as B
from bhusie_amd.layouts import HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH, HIT_UNUSABLE
from tests import accum_filter_ref as FR
from tests import accum_passes_ref as PR

F = np.float32
NAN, INF = F(np.nan), F(np.inf)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _table():
    """(results, records, rays, what): every kind x R.w in {0, -0, 1, -1}, with and without a model slot in the hit word; an unusable record as the device answers it and
    one with stray words; non-finite R in each of x, y, z (NaN, +inf, -inf) and in w alone; iterations around and above 2^24; negative zeros in every input"""
    rows = []

    def row(R, kind, what, slot=0, pos=(1.5, -2.25, 3.0), tri=-1, it=17, closest=2.5, trans=0.75, d=(0.6, -0.0, 0.8)):
        rows.append((R, (kind & 0xFF) | (slot << 8), pos, tri, it, closest, trans, d, what))

    for kind, w in itertools.product((HIT_NONE, HIT_HORIZON, HIT_DISK, HIT_MESH), (0.0, -0.0, 1.0, -1.0)):
        row((0.25, -0.5, 0.125, w), kind, f"kind {kind} w {w}", slot=5 if kind == HIT_MESH else 0, tri=12 if kind == HIT_MESH else -1)
    row((0.0, 0.0, 0.0, -1.0), HIT_UNUSABLE, "unusable", pos=(0.0, 0.0, 0.0), it=0, closest=0.0, trans=0.0, d=(0.0, 0.0, 0.0))
    row((0.0, 0.0, 0.0, -1.0), HIT_UNUSABLE, "unusable with stray words", it=9, d=(0.0, 1.0, 0.0))
    row((0.0, 0.0, 0.0, 0.0), HIT_UNUSABLE, "unusable with alpha 0")
    for ch, bad in itertools.product(range(3), (NAN, INF, -INF)):
        for w in (0.0, 1.0):
            R = [0.25, -0.5, 0.125, w]
            R[ch] = bad
            row(tuple(R), HIT_DISK if w else HIT_NONE, f"R[{ch}] = {bad} w {w}")
    row((0.25, -0.5, 0.125, NAN), HIT_NONE, "w alone is NaN: taken, and NaN == 0 is false")
    row((0.25, -0.5, 0.125, NAN), HIT_DISK, "w alone is NaN, disk")
    row((0.25, -0.5, 0.125, INF), HIT_NONE, "w alone is inf")
    for it in (0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 0x7FFFFFFF, 0x80000001, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF):
        row((0.25, -0.5, 0.125, 1.0), HIT_DISK, f"iterations {it}", it=it)
    row((-0.0, -0.0, -0.0, 0.0), HIT_NONE, "a direction of negative zeros", pos=(-0.0, -0.0, -0.0), closest=-0.0, trans=-0.0, d=(-0.0, -0.0, -0.0))
    row((-0.0, 0.5, -0.0, 1.0), HIT_NONE, "negative zeros in d", d=(-0.0, -0.0, 1.0))
    row((-0.0, 0.5, -0.0, 1.0), HIT_MESH, "negative zeros in the position", pos=(-0.0, 4.0, -0.0), closest=-0.0, trans=-0.0, slot=7, tri=3)
    row((0.5, 0.5, 0.5, 1.0), HIT_HORIZON, "negative zeros where the pass writes zeros", pos=(-0.0, -0.0, -0.0), d=(-0.0, -0.0, -0.0))
    n = len(rows)
    results, records, rays = np.zeros((n, 4), F), np.zeros(n, B.RAY_RECORD_DTYPE), np.zeros((n, 8), F)
    for i, (R, hit, pos, tri, it, closest, trans, d, _) in enumerate(rows):
        results[i] = R
        records[i] = (pos, hit, tri, it, closest, trans)
        rays[i, 0:3] = (9.0, 8.0, 7.0)                            # the origin and the pads are never read
        rays[i, 3] = 5.0
        rays[i, 4:7] = d
        rays[i, 7] = 6.0
    return results, records, rays, [r[-1] for r in rows]


def test_the_host_values_are_the_restatement_in_every_word():
    results, records, rays, what = _table()
    assert len(what) >= 50
    for bit in PR.PASSES:
        got = B.accum_pass_values(results, records, rays, bit)
        want = PR.values(results, records, rays, bit)
        assert got.shape == want.shape == (len(what), 4) and got.dtype == want.dtype == F
        differ = (_bits(got) != _bits(want)).any(axis=1)
        assert not differ.any(), f"pass {bit}: rows {[what[i] for i in np.nonzero(differ)[0]]} differ: {got[differ]} != {want[differ]}"
        if bit != PR.ESCAPE:
            assert np.array_equal(_bits(B.accum_pass_values(results, records, None, bit)), _bits(got)), "rays are read for ESCAPE only"


def test_the_rule_case_by_case():
    """the restatement (and with the test above the library) against the rule written out by hand, row by row"""
    results, records, rays, what = _table()
    v = {bit: PR.values(results, records, rays, bit) for bit in PR.PASSES}
    for i, name in enumerate(what):
        R, q, d = results[i], records[i], rays[i, 4:7]
        kind = int(q["hit"]) & 0xFF
        if not np.isfinite(R[0:3]).all():
            for bit in PR.PASSES:
                assert not _bits(v[bit][i]).any(), f"{name}: a skipped sample is four zero words"
            continue
        zero = [0.0, 0.0, 0.0]
        cov = zero if kind == HIT_UNUSABLE else [float(kind == HIT_HORIZON), float(kind == HIT_DISK), float(kind == HIT_MESH)]
        geo = zero if kind == HIT_UNUSABLE else [q["closest"], F(int(q["iterations"])), q["transmittance"]]
        pos = list(q["position"]) if kind in (HIT_DISK, HIT_MESH) else zero
        esc = zero if kind == HIT_UNUSABLE else list(R[0:3]) if R[3] == 0 else list(d) if kind == HIT_NONE else zero
        for bit, want in ((PR.COVERAGE, cov), (PR.GEOMETRY, geo), (PR.POSITION, pos), (PR.ESCAPE, esc)):
            assert np.array_equal(_bits(v[bit][i]), _bits(np.array(list(want) + [1.0], F))), f"{name}, pass {bit}: {v[bit][i]} != {want}"
    # one rounding to nearest even, above 2^24
    its = {int(q["iterations"]): v[PR.GEOMETRY][i, 1] for i, q in enumerate(records)}
    assert its[(1 << 24) + 1] == F(1 << 24) and its[(1 << 24) + 3] == F((1 << 24) + 4) and its[(1 << 25) + 2] == F(1 << 25) and its[(1 << 25) + 6] == F((1 << 25) + 8)
    assert its[0xFFFFFF7F] == F(0xFFFFFF00) and its[0xFFFFFF80] == F(2.0 ** 32) and its[0xFFFFFFFF] == F(2.0 ** 32) and its[0x80000001] == F(2.0 ** 31)


def test_the_sum_and_the_mean():
    results, records, rays, what = _table()
    n = len(what)
    rng = np.random.default_rng(5)
    per_sample = []
    for s in range(4):                                            # the table's rows dealt to the pixels in another order per sample
        k = rng.permutation(n)
        per_sample.append((results[k], records[k], rays[k]))
    for bit in PR.PASSES:
        total = PR.accumulate(per_sample, bit)
        by_hand = np.zeros((n, 4), F)
        for r, q, d in per_sample:
            by_hand = (by_hand + PR.values(r, q, d, bit)).astype(F)   # a skipped sample adds four zeros
        assert np.array_equal(total[:, 3], by_hand[:, 3]) and np.array_equal(total, by_hand)
        taken = np.sum([PR.taken(r) for r, _, _ in per_sample], axis=0)
        assert np.array_equal(total[:, 3], taken.astype(F)) and (taken < 4).any()
        m = PR.mean(total)
        ok = taken > 0
        assert (m[ok, 3] == 1.0).all() and not m[~ok].any()
        assert np.array_equal(_bits(m[ok, 0:3]), _bits((total[ok, 0:3] / total[ok, 3:4]).astype(F)))
    # the box as a filter is the plain sum; a tent over an image of (v, 1) keeps a constant pass constant where no sample is skipped
    w, h = 6, 5
    q = np.zeros(w * h, B.RAY_RECORD_DTYPE)
    q["hit"] = HIT_DISK; q["closest"] = 3.0; q["iterations"] = 40; q["transmittance"] = 0.5
    r = np.tile(np.array([0.1, 0.2, 0.3, 1.0], F), (w * h, 1))
    flat = [(r, q, None)] * 3
    assert np.array_equal(PR.accumulate(flat, PR.GEOMETRY, FR.Filter(), w, h), PR.accumulate(flat, PR.GEOMETRY))
    tent = PR.mean(PR.accumulate(flat, PR.GEOMETRY, FR.tent(1.5), w, h)).reshape(h, w, 4)
    assert np.allclose(tent[..., 0:3], [3.0, 40.0, 0.5], rtol=1e-6) and (tent[..., 3] == 1.0).all()
