"""CPU: the bound behind which the Cash-Karp step skips its error estimate (bhray_kernels.hip, next_ray_rk_t's SKIP; the proof stands above it).

The kernel forms b = fma(sh*sh, dist, sh*sh) = (dist + 1) * sh^2 from two values the step already holds - dist = |position - hole| and sh = s*h, the
scalar of f times the step size - and, when b <= 3.6e-5 for every active lane of a wave, takes h * 1.0001 without forming e = sum DB_i K_i.  That is the
same step only if no state that passes the bound has e_max above the step-size controller's threshold, 0.00002; the proof gives e_max <= 1.0e-5 for them,
and that - not the threshold - is what is asserted here, on a binary32 restatement of the stages with oracle/np_ray.py's fma32 and constants:
over 2e6 random states (dist log-uniform in [0.5, 1e3], directions uniform - impact parameters from 0, captured, to dist, far -, h log-uniform in [1e-3, 5],
a fifth of them with the hole off the scene's origin, where |position x direction| is not the impact parameter) and over the states along rays of the
default scene at step sizes 0.15 / 1 / 2.  The sample must not be vacuous (a tenth passes, a tenth fails), and a NaN must fail the bound.
"""
import numpy as np
import pytest

import bhusie_amd as B
from oracle import np_ray as N
from tests import common as T

f32 = np.float32
ERR_SKIP_C = f32(3.6e-5)           # bhray_kernels.hip: ERR_SKIP_C
CHUNK = 16384
PROVED = 1.0e-5                    # what the proof bounds e_max by for a state that passes (half the controller's threshold, 0.00002)


def bound_passes(dist, sh):
    """the kernel's test, operation by operation: sh2 = sh*sh; fma(sh2, dist, sh2) <= C (a NaN compares false)"""
    dist = np.asarray(dist, dtype=np.float32); sh = np.asarray(sh, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sh2 = (sh * sh).astype(np.float32)
        return N.fma32(sh2, dist, sh2) <= ERR_SKIP_C


def estimate(pos, dirn, h, bh_pos):
    """(dist, sh, e_max) of one contract step (np_ray.next_ray_rk's stages and error estimate, N3 / N7 / N9 / N10) for states (pos, dirn, h)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        q0 = (pos - bh_pos).astype(np.float32)
        dist = N.flen(q0)
        cr = N.fcross(pos, dirn); h2 = N.fdot(cr, cr)
        sh = (N.f_scale(h2, dist) * h).astype(np.float32)
        shc = sh[:, None]

        def stage(terms):
            acc = q0
            for K, c in terms:
                acc = N.fma32(K, c, acc)
            return (acc * shc).astype(np.float32)

        K1 = (q0 * shc).astype(np.float32)
        K2 = stage([(K1, N.A21)])
        K3 = stage([(K1, N.A31), (K2, N.A32)])
        K4 = stage([(K1, N.A41), (K2, N.A42), (K2, N.A43)])
        K5 = stage([(K1, N.A51), (K2, N.A52), (K3, N.A53), (K4, N.A54)])
        K6 = stage([(K1, N.A61), (K2, N.A62), (K3, N.A63), (K4, N.A64), (K5, N.A65)])
        e = (K1 * N.DB[0]).astype(np.float32)
        for K, c in ((K3, N.DB[2]), (K4, N.DB[3]), (K5, N.DB[4]), (K6, N.DB[5])):
            e = N.fma32(K, c, e)
        ea = np.abs(e)
        return dist, sh, N.fmax(N.fmax(ea[:, 0], ea[:, 1]), ea[:, 2])


def unit_vectors(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def check(dist, sh, e_max, what):
    ok = bound_passes(dist, sh)
    frac = float(ok.mean())
    with np.errstate(invalid="ignore"):
        worst = float(np.max(e_max[ok], initial=0.0))
        bad = ok & ~(e_max <= f32(PROVED))            # a NaN estimate on a passing state counts
    print(f"{what}: {ok.size} states, {100 * frac:.1f} % pass the bound, largest e_max among them {worst:.3g}, over all {float(np.nanmax(e_max)):.3g}")
    assert not bad.any(), f"{what}: {int(bad.sum())} states pass the bound with e_max above {PROVED}: first dist {dist[bad][:3]}, sh {sh[bad][:3]}, e_max {e_max[bad][:3]}"
    return frac


def test_random_states_that_pass_the_bound_have_a_small_estimate():
    rng = np.random.default_rng(11)
    n = 2_000_000
    dist = np.exp(rng.uniform(np.log(0.5), np.log(1e3), n))
    h = np.exp(rng.uniform(np.log(1e-3), np.log(5.0), n)).astype(np.float32)
    bh_pos = np.zeros((n, 3), dtype=np.float32)
    off = rng.random(n) < 0.2
    bh_pos[off] = rng.uniform(-8.0, 8.0, (int(off.sum()), 3)).astype(np.float32)
    pos = (unit_vectors(rng, n).astype(np.float64) * dist[:, None] + bh_pos).astype(np.float32)
    dirn = unit_vectors(rng, n)
    parts = [estimate(pos[i:i + CHUNK], dirn[i:i + CHUNK], h[i:i + CHUNK], bh_pos[i:i + CHUNK]) for i in range(0, n, CHUNK)]      # (chunks that stay in the cache: 3x faster)
    d, sh, e_max = (np.concatenate([p[k] for p in parts]) for k in range(3))
    assert 0.45 <= float(d.min()) and float(d.max()) <= 1.1e3
    b = np.sqrt(N.fdot(N.fcross(pos - bh_pos, dirn), N.fcross(pos - bh_pos, dirn)))
    assert float(b.min()) < 0.5 and float(b.max()) > 100.0, "impact parameters: captured and far rays"
    frac = check(d, sh, e_max, "random states")
    assert 0.1 <= frac <= 0.9, f"vacuous sample: {frac:.3f} of the states pass the bound"
    with np.errstate(invalid="ignore"):
        assert (e_max > f32(0.00002)).mean() > 0.05, "the sample never takes the step-size power's arm"


@pytest.mark.parametrize("step_size", [0.15, 1.0, 2.0])
def test_states_along_rays_of_the_default_scene(step_size):
    """every step of a 48 x 27 grid of rays of the default scene (camera inside the sphere, hole at the origin), marched with np_ray.next_ray_rk until the ray leaves
    the sphere, comes within the horizon's radius or has taken 400 steps"""
    u = T.uniforms(integration_method=1, step_size=step_size)
    S = N.Scene(*u, *T.textures())
    w, hgt = 48, 27
    py, px = np.mgrid[0:hgt, 0:w]
    pos, dirn = N.create_rays(S, px.ravel(), py.ravel(), w, hgt)
    h = np.full(pos.shape[0], S.step_size, dtype=np.float32)
    bh = np.broadcast_to(S.bh_pos, pos.shape)
    ds, shs, es = [], [], []
    for _ in range(400):
        if pos.shape[0] == 0:
            break
        d, sh, e_max = estimate(pos, dirn, h, bh[:pos.shape[0]])
        ds.append(d); shs.append(sh); es.append(e_max)
        pos, dirn, h = N.next_ray_rk(S, pos, dirn, h)
        cd = N.flen(pos - S.bh_pos)
        with np.errstate(invalid="ignore"):
            keep = (cd <= S.R) & (cd > f32(1.0)) & np.isfinite(cd)
        pos, dirn, h = pos[keep], dirn[keep], h[keep]
    d, sh, e_max = np.concatenate(ds), np.concatenate(shs), np.concatenate(es)
    assert d.size > 10_000
    frac = check(d, sh, e_max, f"default scene, step_size {step_size}")
    assert frac > 0.3, "the bound holds on the bulk of a real scene's steps"
    if step_size >= 1.0:
        assert (e_max > f32(0.00002)).any(), "this scene takes the step-size power's arm"


def test_a_nan_fails_the_bound():
    nan, inf = f32(np.nan), f32(np.inf)
    assert bound_passes(f32(5.0), f32(1e-4)) and bound_passes(f32(0.0), f32(0.0)) and bound_passes(f32(1e3), f32(-1e-4))
    assert not bound_passes(nan, f32(1e-4)) and not bound_passes(nan, f32(0.0))
    assert not bound_passes(f32(5.0), nan) and not bound_passes(nan, nan)
    assert not bound_passes(inf, f32(1e-4)) and not bound_passes(inf, f32(0.0))          # inf * 0 = NaN
    assert not bound_passes(f32(5.0), inf) and not bound_passes(f32(5.0), -inf) and not bound_passes(f32(5.0), f32(3e38))
    assert not bound_passes(f32(5.0), f32(0.0061)) and not bound_passes(f32(1e3), f32(2e-4))
    d = np.array([5.0, np.nan, 5.0, 1.0], dtype=np.float32); s = np.array([1e-4, 1e-4, np.nan, 1.0], dtype=np.float32)
    assert bound_passes(d, s).tolist() == [True, False, False, False]


def test_the_constants_of_the_proof():
    """sum_i |DB_i| * sum_j |a_ij| <= 0.2492, |sum DB_i| <= 1.5e-9, the largest row sum of |a| <= 6.593: the figures the comment above next_ray_rk_t uses"""
    rows = [[], [N.A21], [N.A31, N.A32], [N.A41, N.A42, N.A43], [N.A51, N.A52, N.A53, N.A54], [N.A61, N.A62, N.A63, N.A64, N.A65]]
    R = [sum(abs(float(a)) for a in r) for r in rows]
    db = [float(v) for v in N.DB]
    assert db[1] == 0.0
    assert abs(sum(db)) <= 1.5e-9
    assert max(R) <= 6.593
    assert sum(abs(c) * r for c, r in zip(db, R)) <= 0.2492
    assert sum(abs(c) for c in db) <= 0.1156
    k = 1.0 / (1.0 - 6.593 * 0.006)
    assert k <= 1.0412 and 0.2492 * k <= 0.2595
    assert 0.2595 * 3.6e-5 + 1.02e-7 * np.sqrt(3.6e-5 * 1e6) <= PROVED
