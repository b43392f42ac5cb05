"""-m gpu: adaptive stills - each pixel sampled until the error of its mean is under a bound (bhray_accum_add_adaptive).

  1. The mean, the counts and the divisor equal the restatement (tests/accum_adaptive_ref.py) over the device's own trace results, in every word; the frame splits.
  2. The selection after the first round is the restatement's set; a huge tolerance, a zero tolerance, a tolerance that fails exactly one pixel.
  3. Against §18 without the restatement: a huge tolerance is accum_add(min_samples); the pixels that reach max_samples carry accum_add(max_samples)'s words.
  4. The cut of a round into launches and of the work into calls changes no word; begin clears, the counts included.
  5. A second call with half the tolerance continues; info and accum_samples.
  6. Samples that are not finite: the test uses the samples taken.
  7. The mean against the oracle's trace_ray of exactly the samples each pixel took.
  8. The refused states, the two modes, bad parameters; frames keep their bits; a model upload waits.
  9. The display read, Renderer.render_still(adaptive=...), bhray_render --spp-adaptive.

The frames are tests/test_gpu_accum.py's: ladder_for_frame((40, 36), 3, 2) - 1 440 pixels, no multiple of 64 or 256, six blocks of the selection kernel, the last one partly
filled - and one 33 x 32 single-level frame.  Parameters: accum_adaptive_ref.GPU_TEST (min 4 / round 4 / max 12; the tolerance chosen on the CPU from the oracle)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from tests import accum_adaptive_ref as R
from tests import accum_ref as A
from tests import common as T
from tests import post_ref as P
from tests import rays_ref as RR

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
CFGS = {"40x36_of_a_ladder": lambda: B.ladder_for_frame((40, 36), 3, 2), "33x32_one_level": lambda: B.ladder_from_base((33, 32), 3, 1)}
CAM = B.Camera()
FAR = B.Camera(position=(2.0, 1.0, -45.0), forward=(0.0, 0.0, 1.0), fov=0.9)          # tests/test_gpu_accum.py's hole-away scene: NaN colours on the far rim
HOLE_AWAY_NAN = B.BlackHole(position=(1.5, -0.75, 2.0))
MESH_CAM = B.Camera(position=(0.0, 0.0, -60.0), forward=(-0.1, 0.0, 1.0), fov=1.0)
MESH_AT = (-22.0, 4.0, -25.0)
G = R.GPU_TEST
K = G.as_kwargs()
HUGE = 1e30


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(cfg=None, **kw):
    rp = B.RayPass(cfg if cfg is not None else CFGS["40x36_of_a_ladder"](), **({"device": 0} if "devices" not in kw else {}), **kw)
    rp.set_textures(*T.textures())
    return rp


def _code(call):
    with pytest.raises(B.BhrayError) as e:
        call()
    return e.value.code


def _kw(**over):
    return {**K, **over}


@functools.lru_cache(maxsize=None)
def _scene(shape, method, far=False):
    """(ray pass under the scene's uniforms, the DEVICE's trace results for the restatement's rays of samples 0 .. 11): computed once, left unchanged"""
    rp = _ctx(CFGS[shape]())
    cam = FAR if far else CAM
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=method, **({"black_hole": HOLE_AWAY_NAN} if far else {})))
    res = [rp.trace_rays(A.sample_rays(cam, rp.cfg, s)) for s in range(G.max_samples)]
    for r in res:
        r.setflags(write=False)
    return rp, res


def _restate(res, *params):
    st = R.State(res[0].shape[0])
    out = [R.call(st, p, res, T.textures()[2]) for p in params]
    return st, out


def _image(rp):
    return rp.accum_read().reshape(-1, 4), rp.accum_read_counts().reshape(-1)


def _adaptive(rp, *kws):
    rp.accum_begin()
    infos = [rp.accum_add_adaptive(**kw) for kw in kws]
    return _image(rp) + (infos,)


def _same(got, want, what):
    differ = int((_bits(got) != _bits(want)).sum())
    assert differ == 0, f"{what}: {differ} of {np.asarray(want).size} words differ"


# ---- 1. to the bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_image_and_the_counts_are_the_restatements(shape, method):
    rp, res = _scene(shape, method)
    st, ((info, actives),) = _restate(res, G)
    npix = st.issued.size
    assert npix % 64 != 0
    stop, more, top = float((st.issued == 4).mean()), float((st.issued > 4).mean()), int((st.issued == 12).sum())
    print(f"{shape} method {method}: {100 * stop:.1f} % stop at 4, {100 * more:.1f} % take more, {top} of {npix} reach 12; rounds {info['rounds']}, rays {info['rays']}")
    assert stop >= 0.10 and more >= 0.10 and top >= 1, "the frame must split: pixels that stop at once, pixels that go on, a pixel at max_samples"
    mean, counts, (got_info,) = _adaptive(rp, K)
    assert mean.dtype == np.float32 and counts.dtype == np.uint32 and rp.accum_read_counts().shape == (rp.cfg.frame_h, rp.cfg.frame_w)
    assert np.array_equal(counts, st.issued), f"{int((counts != st.issued).sum())} counts differ"
    _same(mean, R.mean(st), "the mean")
    assert (st.sum[:, 3] == st.issued).all() and (mean[:, 3] == 1.0).all(), "the default scene skips no sample: the divisor is the count"
    assert got_info == info


# ---- 2. selection -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_selection_is_the_restatements_set(method):
    rp, res = _scene("40x36_of_a_ladder", method)
    first = R.Params(4, 4, 4, G.tolerance, G.dark)                # max = min: the first round and nothing else
    st, _ = _restate(res, first)
    rp.accum_begin()
    info = rp.accum_add_adaptive(**first.as_kwargs())
    assert info == {"rounds": 1, "active_last": 0, "rays": 4 * st.issued.size, "reach": 4}
    got = rp.accum_active_pixels(**K)
    want = R.select(st, G)
    assert want.size >= 0.10 * st.issued.size
    assert len(set(got.tolist())) == got.size, "a pixel occurs twice in the list"
    assert np.array_equal(np.sort(got), want), "the compacted list is not the restatement's set"
    assert rp.accum_active_pixels(**_kw(tolerance=HUGE)).size == 0
    assert rp.accum_active_pixels(**_kw(max_samples=4)).size == 0, "every pixel is at max_samples"
    with np.errstate(invalid="ignore", divide="ignore"):
        n = st.sum[:, 3]
        m, q = st.S1 / n, st.S2 / n
        v = (q - (m * m).astype(np.float32)).astype(np.float32)
    varied = np.nonzero(~(v <= 0))[0]                             # v > 0, or a NaN
    assert 0 < varied.size < st.issued.size
    assert np.array_equal(np.sort(rp.accum_active_pixels(**_kw(tolerance=0.0, dark=0.0))), varied), "tolerance 0: every pixel of non-zero variance"
    # a tolerance between the two largest ratios sqrt(v / n) / (m + dark): exactly one pixel fails - decided by the restatement, not assumed
    ratio = np.sqrt(np.maximum(v, 0).astype(np.float64) / n) / (m.astype(np.float64) + float(G.dark))
    order = np.argsort(ratio)
    one = R.Params(4, 12, 4, np.sqrt(ratio[order[-1]] * ratio[order[-2]]), G.dark)
    assert R.select(st, one).tolist() == [int(order[-1])]
    assert rp.accum_active_pixels(**one.as_kwargs()).tolist() == [int(order[-1])]
    _same(rp.accum_read_counts().reshape(-1), np.full(st.issued.size, 4, np.uint32), "a selection changed the counts")


# ---- 3. against §18 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("shape", list(CFGS))
def test_against_the_uniform_accumulation(shape, method):
    rp, _ = _scene(shape, method)
    uniform = {}
    for S in (G.min_samples, G.max_samples):
        rp.accum_begin(); rp.accum_add(S)
        uniform[S] = rp.accum_read().reshape(-1, 4)
    mean, counts, (info,) = _adaptive(rp, _kw(tolerance=HUGE))
    assert (counts == 4).all() and info["rounds"] == 1 and rp.accum_samples() == 4
    _same(mean, uniform[4], "a huge tolerance against accum_add(min_samples)")
    mean, counts, (info,) = _adaptive(rp, _kw(tolerance=0.0, dark=0.0))
    full = counts == 12
    assert full.any() and (counts == 4).any() and info["reach"] == 12
    _same(mean[full], uniform[12][full], "the pixels at max_samples against accum_add(max_samples)")


# ---- 4. grouping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_cut_into_launches_and_calls_changes_no_word(method):
    rp, _ = _scene("40x36_of_a_ladder", method)
    npix = int(rp.cfg.frame_w) * int(rp.cfg.frame_h)
    whole, counts, (info,) = _adaptive(rp, K)
    try:
        for launch_rays in (npix, 64):                            # one sub-sample of the first round per launch; rounds cut into chunks of one sub-sample
            rp.accum_set_launch_rays(launch_rays)
            m, c, (i,) = _adaptive(rp, K)
            _same(m, whole, f"launch_rays {launch_rays}: the mean"); _same(c, counts, f"launch_rays {launch_rays}: the counts")
            assert i == info
    finally:
        rp.accum_set_launch_rays(0)
    m, c, (ia, ib) = _adaptive(rp, _kw(max_samples=8), K)
    _same(m, whole, "max 8 then max 12: the mean"); _same(c, counts, "max 8 then max 12: the counts")
    assert ia["reach"] == 8 and ib["reach"] == 12 and ia["rays"] + ib["rays"] == info["rays"] and ia["rounds"] + ib["rounds"] == info["rounds"]
    rp.accum_begin()                                              # clears: the sum, the moments, the counts
    assert rp.accum_samples() == 0 and not rp.accum_read().any()
    assert np.array_equal(np.sort(rp.accum_active_pixels(**K)), np.arange(npix)), "after begin every pixel has n = 0 and issued = 0: all are selected"
    m, c, _ = _adaptive(rp, K)
    _same(m, whole, "after begin: the mean"); _same(c, counts, "after begin: the counts")


# ---- 5. continuation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_a_second_call_with_half_the_tolerance_continues(method):
    rp, res = _scene("40x36_of_a_ladder", method)
    first, second = R.Params(4, 12, 4, 2 * float(G.tolerance), G.dark), G
    st, ((i1, _), (i2, a2)) = _restate(res, first, second)
    assert i2["rounds"] >= 1 and i2["rays"] > 0, "the second call must have work"
    rp.accum_begin()
    g1 = rp.accum_add_adaptive(**first.as_kwargs())
    assert rp.accum_samples() == g1["reach"]
    g2 = rp.accum_add_adaptive(**second.as_kwargs())
    assert (g1, g2) == (i1, i2) and g2["active_last"] == 0
    assert rp.accum_samples() == g2["reach"] == int(st.issued.max())
    mean, counts = _image(rp)
    _same(counts, st.issued, "the counts"); _same(mean, R.mean(st), "the mean")
    assert _code(lambda: rp.accum_add_adaptive(**_kw(min_samples=2, max_samples=12, round_samples=2))) == E_INVALID, "min / round must repeat the first call's"
    assert _code(lambda: rp.accum_add_adaptive(**_kw(round_samples=8))) == E_INVALID
    _same(rp.accum_read_counts().reshape(-1), st.issued, "a refused call changed the counts")


# ---- 6. skipped samples -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_samples_that_are_not_finite(method):
    rp, res = _scene("40x36_of_a_ladder", method, far=True)
    st, ((info, _),) = _restate(res, G)
    n = st.sum[:, 3]
    short = n < st.issued
    print(f"method {method}: {int(short.sum())} pixels took fewer samples than were issued; issued {dict(zip(*np.unique(st.issued, return_counts=True)))}")
    assert short.any(), "the scene must produce samples that are not finite"
    by_issued = R.State(n.size)                                   # what a test that divided by issued would have selected after the first round (reported, not asserted)
    after4, _ = _restate(res, R.Params(4, 4, 4, G.tolerance, G.dark))
    by_issued.sum, by_issued.S1, by_issued.S2, by_issued.issued = after4.sum.copy(), after4.S1, after4.S2, after4.issued
    by_issued.sum[:, 3] = 4.0
    print(f"  first selection: {R.select(after4, G).size} pixels by n, {R.select(by_issued, G).size} by issued")
    mean, counts, (got,) = _adaptive(rp, K)
    assert np.isfinite(mean).all(), "a NaN sample reached the mean"
    assert np.array_equal(mean[:, 3] == 0.0, n == 0)
    _same(counts, st.issued, "the counts"); _same(mean, R.mean(st), "the mean")
    assert got == info


# ---- 7. oracle ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_samples(method):
    cfg = CFGS["40x36_of_a_ladder"]()
    sc = T.oracle_scene(*T.uniforms(camera=CAM, integration_method=method), T.textures())
    return [RR.oracle_rays(sc, A.sample_rays(CAM, cfg, s))[0] for s in range(G.max_samples)]


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_the_mean_against_the_oracle(method):
    rp, _ = _scene("40x36_of_a_ladder", method)
    got, counts, _ = _adaptive(rp, K)
    per_sample = _oracle_samples(method)
    assert all(np.isfinite(r).all() for r in per_sample)
    want = np.zeros_like(got)
    for S in np.unique(counts):                                   # exactly the samples each pixel took: 0 .. S - 1, S the device's count
        k = counts == S
        want[k] = A.mean(A.accumulate([r[k] for r in per_sample[:int(S)]], T.textures()[2]))
    assert np.array_equal(got[:, 3], want[:, 3])
    bar = 2 * T.REL_TOL + (counts.astype(np.float64) + 1) * 2.0 ** -23          # §18's bar with S the pixel's own count
    err = T.rel_err(got[:, 0:3], want[:, 0:3]).max(axis=1)
    print(f"method {method}: max rel err {float(err.max()):.3g} (bars {float(bar.min()):.3g} .. {float(bar.max()):.3g}), counts {dict(zip(*np.unique(counts, return_counts=True)))}")
    assert (err <= bar).all(), f"max rel err {float(err.max()):.3g}"


# ---- 8. states ----------------------------------------------------------------------------------------
def _raw(rp, a):
    return rp._L.bhray_accum_add_adaptive(rp._h, C.byref(a) if a is not None else None, None)


def test_refused_states_modes_and_bad_parameters():
    u = T.uniforms(camera=CAM, integration_method=1)
    rp = _ctx()
    assert _code(lambda: rp.accum_add_adaptive(**K)) == E_STATE   # before begin
    assert _code(rp.accum_read_counts) == E_STATE and _code(lambda: rp.accum_active_pixels(**K)) == E_STATE
    rp.accum_begin()
    assert _code(lambda: rp.accum_add_adaptive(**K)) == E_STATE   # before the first set_uniforms
    rp.set_uniforms(*u)
    assert _code(rp.accum_read_counts) == E_STATE, "no adaptive call yet"
    rp.set_mesh_lensing(True)
    assert _code(lambda: rp.accum_add_adaptive(**K)) == E_STATE
    rp.set_mesh_lensing(False)
    rp.accum_add_adaptive(**K)
    mean, counts = _image(rp)
    assert _code(lambda: rp.accum_add(1)) == E_STATE, "accum_add after an adaptive call"
    good = layouts.BhrayAccumAdaptive(C.sizeof(layouts.BhrayAccumAdaptive), 4, 12, 4, 0.0, 0.0)    # tolerance 0: a call that passed would sample on
    assert _raw(rp, None) == E_INVALID
    for field, value in (("struct_size", 20), ("struct_size", 0), ("min_samples", 1), ("min_samples", 0), ("max_samples", 3), ("max_samples", 65540), ("max_samples", 13),
                         ("round_samples", 0), ("tolerance", float("nan")), ("tolerance", float("inf")), ("tolerance", -0.5), ("dark", float("nan")),
                         ("dark", float("-inf")), ("dark", -1e-3)):
        bad = layouts.BhrayAccumAdaptive.from_buffer_copy(good)
        setattr(bad, field, value)
        assert _raw(rp, bad) == E_INVALID, (field, value)
        n = C.c_uint32(77)
        assert rp._L.bhray_accum_active_pixels(rp._h, C.byref(bad), None, 0, C.byref(n)) == E_INVALID and n.value == 77, (field, value)
    m2, c2 = _image(rp)
    _same(m2, mean, "bad parameters touched the sum"); _same(c2, counts, "bad parameters touched the counts")
    assert rp.accum_samples() == int(counts.max())
    rp.accum_begin()                                              # resets the mode
    rp.accum_add(2)
    assert _code(lambda: rp.accum_add_adaptive(**K)) == E_STATE, "adaptive after accum_add"
    assert _code(rp.accum_read_counts) == E_STATE and _code(lambda: rp.accum_active_pixels(**K)) == E_STATE, "the counts of a uniform accumulation"
    rp.accum_add(1)
    assert rp.accum_samples() == 3
    rp.accum_begin()
    rp.accum_add_adaptive(**K)
    m3, c3 = _image(rp)
    _same(m3, mean, "begin must reset the mode and the image"); _same(c3, counts, "the counts")
    for kw in ({"literal": True}, {"eval_fma": True}, {"devices": [0, 0]}, {"row_rank": 0, "row_world": 2}):
        q = _ctx(**kw)
        q.set_uniforms(*u)
        assert _code(q.accum_begin) == E_STATE, kw
        assert _code(lambda: q.accum_add_adaptive(**K)) == E_STATE, kw
        assert _code(q.accum_read_counts) == E_STATE and _code(lambda: q.accum_active_pixels(**K)) == E_STATE, kw
        assert q.accum_samples() == 0


def test_frames_before_and_after_keep_their_bits():
    u = T.uniforms(camera=CAM, integration_method=1)
    plain = _ctx()
    plain.set_uniforms(*u)
    plain.render()
    frame = plain.read_hdr().copy()
    alone, alone_counts, _ = _adaptive(plain, K)
    rp = _ctx()
    rp.set_uniforms(*u)
    rp.render()
    rp.accum_begin(); rp.accum_add_adaptive(**K)                  # behind a frame in flight
    rp.render()
    second = rp.read_hdr().copy()
    mixed, mixed_counts = _image(rp)
    rp.render()
    assert np.array_equal(_bits(second), _bits(frame)) and np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed with an adaptive accumulation beside it"
    _same(mixed, alone, "the accumulation between two frames"); _same(mixed_counts, alone_counts, "its counts")


def test_a_model_upload_waits_for_an_outstanding_adaptive_accumulation():
    old, new = RR.mesh_model(MESH_AT), RR.mesh_model((0.0, -30.0, 5.0))
    rp = _ctx()
    rp.upload_model(old)
    rp.set_uniforms(*T.uniforms(camera=MESH_CAM, integration_method=1, model_count=1))
    want_old, counts_old, _ = _adaptive(rp, K)
    rp.accum_begin()
    rp.accum_add_adaptive(**K)
    rp.upload_model(new)                                          # with the last round outstanding: must wait for it, not pull the old model from under it
    got, counts = _image(rp)
    _same(got, want_old, "the outstanding accumulation did not see the OLD model"); _same(counts, counts_old, "its counts")
    want_new, _, _ = _adaptive(rp, K)
    assert int((_bits(want_new) != _bits(want_old)).any(axis=1).sum()) >= 20, "the two models must differ in the image"
    rp.sync()


# ---- 9. hosts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_display_read_is_post_ref_of_the_rounded_mean(shape):
    rp, _ = _scene(shape, 1)
    rp.accum_begin(); rp.accum_add_adaptive(**K)
    mean = rp.accum_read()
    disp = rp.accum_read_display()
    assert disp.shape == (rp.cfg.frame_h, rp.cfg.frame_w, 4) and disp.dtype == np.uint8
    with np.errstate(over="ignore"):
        sky16 = mean.astype(np.float16)                           # nearest even
    assert np.array_equal(disp, P.post_ref(sky16)), "the display read differs from post_ref over the binary16 mean"
    _same(rp.accum_read(), mean, "the display read changed the mean")


def test_render_still_adaptive_is_the_ray_pass_calls():
    r = B.Renderer(CFGS["40x36_of_a_ladder"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    r.ray_details.time = 0.5
    rp = _ctx()
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    rp.accum_begin(); rp.accum_add(16)
    _same(r.render_still(), rp.accum_read(), "render_still() without the argument: 16 uniform samples, as before")
    assert r.still_info is None and _code(r.still_counts) == E_STATE
    still = r.render_still(adaptive=B.AdaptiveStill(**K))
    want, want_counts, (info,) = _adaptive(rp, K)
    assert still.shape == (36, 40, 4) and still.dtype == np.float32
    _same(still.reshape(-1, 4), want, "render_still(adaptive=...)"); _same(r.still_counts().reshape(-1), want_counts, "still_counts()")
    assert r.still_info == info and r.ray_pass.accum_samples() == info["reach"]
    _same(r.render_still(samples=4), _uniform(rp, 4), "a uniform still after an adaptive one")


def _uniform(rp, S):
    rp.accum_begin(); rp.accum_add(S)
    return rp.accum_read()


def test_cpp_host_writes_an_adaptive_still(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / "still.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "14", "13", "--levels", "2", "--disk-size", "64", "--spp-adaptive", "4", "12", "0.05", "--spp-dark", "0.01"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "40x37"
    got = np.fromfile(out, dtype=np.float32).reshape(37, 40, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(B.ladder_from_base((14, 13), 3, 2), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    want = r2.render_still(adaptive=B.AdaptiveStill(4, 12, 4, 0.05, 0.01))
    _same(got, want, "the C++ host's adaptive still against the Python host's")
    counts = r2.still_counts()
    assert lines[-1] == "adaptive rounds=%u rays=%u mean_count=%.6f" % (r2.still_info["rounds"], r2.still_info["rays"], float(counts.astype(np.float64).sum()) / counts.size)
    assert len(np.unique(counts)) >= 2, "the still must be adaptive in fact"
