"""-m gpu: the moving observer of stills - Lorentz aberration of every generated ray, Doppler beaming of every resolved sample (bhray_accum_set_observer).

Every bit-for-bit comparison is against NumPy over the device's OWN trace results for the host-form rays (bhray_observer_sample_rays_host, which the CPU tests hold to
tests/observer_ref.py), so nothing of it depends on how the rays were traced.

   1. bhray_accum_sample_rays under an observer equals the host form in every word: four cameras, both shapes, s in {0, 1, 7}.
   2. The box mean equals NumPy in every word: beaming on and off, 5 samples in one call and as 3 + 2, a launch boundary inside the call.
   3. The same under a tent filter.
   4. The same under the equirect camera with point stars on a whole-width frame, beaming on: the star stage saw unbeamed direction pixels, the starred pixels are beamed.
   5. Adaptive: mean, counts and every round's selection are tests/accum_adaptive_ref.py's fed the beamed samples.
   6. Lensed meshes in stills (BHRAY_LENS_FRAMES | BHRAY_LENS_RAYS) under an observer.
   7. An observer set and cleared, by NULL or by a zero velocity, leaves an accumulation bit-identical; frames and ray batches keep their bits while one is set;
      a refused observer leaves the one in force.
   8. Against the oracle: a 24 x 16 equirect still of 2 samples, beta = (0.4, 0, 0.2), beaming on, at tests/test_gpu_still_camera.py's bar.
   9. Physics: from the disk's axis, the number of first hits on the horizon falls strictly over beta = -0.5, 0, +0.5 along forward.
  10. The display read succeeds under an observer.
  11. Renderer.render_still(observer=...) equals the RayPass sequence.
  12. bhray_render --spp 2 --observer 0.5 0 0 writes another image than without the flag.

Frames: 48 x 32 and 37 x 33 with levels = 1 - 1 536 pixels (six blocks of 256) and 1 221 (no multiple of 64, a partial last block)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras
from bhusie_amd.cameras import Observer, StillCamera
from bhusie_amd.renderer import StillFilter
from tests import accum_adaptive_ref as AR
from tests import accum_filter_ref as FR
from tests import accum_ref as A
from tests import accum_stars_ref as AS
from tests import common as T
from tests import observer_ref as OR
from tests import post_ref as P
from tests import rays_ref as RR
from tests import stars_ref as S
from tests import test_gpu_lensed as GL

pytestmark = pytest.mark.gpu

E_INVALID = -1
CFGS = {"48x32": lambda: B.ladder_from_base((48, 32), 3, 1), "37x33": lambda: B.ladder_from_base((37, 33), 3, 1)}
CAMERAS = {"pinhole": StillCamera.pinhole(), "equirect": StillCamera.equirect(), "fisheye": StillCamera.fisheye(3.4), "lens": StillCamera.pinhole(lens_radius=0.3, focus_distance=12.0)}
# tests/test_gpu_still_camera.py's cameras: inside the disk's outer radius for the panorama and the fisheye, further out for the pinhole and the lens
NEAR = B.Camera(position=(0.0, 1.5, -6.0), forward=(0.0, -0.25, 1.0), fov=1.3)
LENS_CAM = B.Camera(position=(0.0, 2.0, -12.0), forward=(0.0, -0.16, 1.0), fov=1.3)
SCENE_CAM = {"pinhole": LENS_CAM, "equirect": NEAR, "fisheye": NEAR, "lens": LENS_CAM}
VEL = (0.5, 0.0, 0.0)
VEL2 = (0.0, -0.3, 0.2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(cfg=None):
    rp = B.RayPass(cfg if cfg is not None else CFGS["48x32"](), device=0)
    rp.set_textures(*T.textures())
    return rp


def _npix(cfg):
    return int(cfg.frame_w) * int(cfg.frame_h)


def _accumulate(rp, groups):
    rp.accum_begin()
    for g in groups:
        rp.accum_add(g)
    return rp.accum_read()


def _host(cfg, cam_bytes, still, observer, s):
    """(records, beam) of bhray_observer_sample_rays_host"""
    n = _npix(cfg)
    out, beam = np.empty((n, 8), dtype=np.float32), np.empty(n, dtype=np.float32)
    st = still.struct() if still is not None else None
    ob = observer.struct() if observer is not None else None
    rc = B.lib().bhray_observer_sample_rays_host(C.byref(cfg), cam_bytes, C.byref(st) if st is not None else None, C.byref(ob) if ob is not None else None, int(s),
                                                 out.ctypes.data, beam.ctypes.data)
    assert rc == 0, rc
    return out, beam


def _trace(rp, rec):
    """the device's trace results for the records; a record without a direction (a fisheye sample outside the circle) is left out and entered as (0, 0, 0, -1)"""
    usable = (rec[:, 4:7] != 0.0).any(axis=1)
    out = np.zeros((rec.shape[0], 4), np.float32)
    out[:, 3] = -1.0
    out[usable] = rp.trace_rays(np.ascontiguousarray(rec[usable]))
    return out


def _beamed(results, rec, beam, sky, on=True):
    """the beam stage in NumPy: a direction pixel is resolved, the colour of every record with a direction is multiplied by its beam, alpha is kept"""
    if not on:
        return np.asarray(results, np.float32).reshape(-1, 4).copy()
    v = A.resolve(results, sky)
    live = (rec[:, 4:7] != 0.0).any(axis=1)
    raw = np.asarray(results, np.float32).reshape(-1, 4)
    v[~live] = raw[~live]
    with np.errstate(over="ignore", invalid="ignore"):
        v[live, 0:3] = (v[live, 0:3] * beam[live, None]).astype(np.float32)
    return v


def _samples(rp, cam, still, observer, n):
    """[(results, records, beam)] of samples 0 .. n - 1: the host-form rays traced on the device"""
    out = []
    for s in range(n):
        rec, beam = _host(rp.cfg, cam.uniform(), still, observer, s)
        out.append((_trace(rp, rec), rec, beam))
    return out


def _assert_words(got, want, what):
    differ = int((_bits(np.asarray(got).reshape(-1, 4)) != _bits(np.asarray(want).reshape(-1, 4))).sum())
    print(f"{what}: {differ} of {np.asarray(want).size} words differ")
    assert differ == 0, f"{what}: {differ} of {np.asarray(want).size} words differ from NumPy over the device's results"


# ---- 1. records -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(CAMERAS))
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_generated_records_are_the_host_forms(shape, kind):
    cam = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=cam))
    rp.accum_set_camera(CAMERAS[kind])
    plain = rp.accum_sample_rays(1)
    for vel in (VEL, VEL2):
        rp.accum_set_observer(vel)
        for s in (0, 1, 7):
            got, (want, _) = rp.accum_sample_rays(s), _host(rp.cfg, cam.uniform(), CAMERAS[kind], Observer(vel), s)
            differ = int((_bits(got) != _bits(want)).sum())
            assert differ == 0, f"{kind} {vel} sample {s}: {differ} of {got.size} words differ from the host form"
        assert not np.array_equal(_bits(rp.accum_sample_rays(1)), _bits(plain)), "the observer must change the records"
    rp.accum_set_observer(None)
    assert np.array_equal(_bits(rp.accum_sample_rays(1)), _bits(plain)), "NULL restores the still camera's generator"
    rp.close()


# ---- 2. the box mean, to the bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("beaming", [True, False], ids=["beamed", "aberration_only"])
@pytest.mark.parametrize("kind", list(CAMERAS))
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_box_mean_is_numpy_over_the_devices_own_results(shape, kind, beaming):
    n = 5
    cam, still, sky = SCENE_CAM[kind], CAMERAS[kind], T.textures()[2]
    rp = _ctx(CFGS[shape]())
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=1))
    per = _samples(rp, cam, still, Observer(VEL, beaming), n)
    want = A.mean(A.accumulate([_beamed(r, rec, beam, sky, beaming) for r, rec, beam in per], sky))
    rp.accum_set_camera(still)
    plain = _accumulate(rp, [n])
    rp.accum_set_observer(VEL, beaming)
    rp.accum_set_launch_rays(2 * _npix(rp.cfg))                   # two samples per launch: 2 + 2 + 1, a launch boundary inside the call
    got = _accumulate(rp, [n])
    assert rp.accum_samples() == n
    _assert_words(got, want, f"{shape} {kind} beaming {beaming}, add(5)")
    _assert_words(_accumulate(rp, [3, 2]), want, f"{shape} {kind} beaming {beaming}, add(3); add(2)")
    rp.accum_set_launch_rays(0)
    _assert_words(_accumulate(rp, [n]), want, f"{shape} {kind} beaming {beaming}, one launch")
    assert int((_bits(got) != _bits(plain)).any(axis=-1).sum()) >= 100, "the observer must change the image"
    if beaming:
        sky0 = per[0][0][:, 3] == 0.0
        assert sky0.sum() >= 10 and (per[0][2][sky0] != 1.0).any(), "direction pixels with a beam other than 1"
        rp.accum_set_observer(VEL, False)
        assert not np.array_equal(_bits(_accumulate(rp, [n])), _bits(got)), "beaming must change the image"
    rp.close()


# ---- 3. under a tent ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_tent_filtered_mean(shape):
    n = 5
    cam, sky = LENS_CAM, T.textures()[2]
    rp = _ctx(CFGS[shape]())
    w, h = int(rp.cfg.frame_w), int(rp.cfg.frame_h)
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=1))
    per = _samples(rp, cam, None, Observer(VEL2), n)
    beamed = [_beamed(r, rec, beam, sky) for r, rec, beam in per]
    want = A.mean(FR.accumulate(beamed, sky, FR.tent(1.5), w, h))
    rp.accum_set_filter(StillFilter.tent(1.5))
    rp.accum_set_observer(VEL2)
    rp.accum_set_launch_rays(2 * w * h)
    _assert_words(_accumulate(rp, [n]), want, f"{shape} tent, add(5)")
    # the second call starts at sample 3: its weights are those of samples 3 and 4
    _assert_words(_accumulate(rp, [3, 2]), want, f"{shape} tent, add(3); add(2)")
    rp.close()


# ---- 4. equirect with point stars -------------------------------------------------------------------------------
def test_the_equirect_still_with_point_stars():
    n = 2
    cam, bh = S.scene("default")
    sky, cat = T.textures()[2], S.catalogue()
    rp = _ctx()
    w, h = int(rp.cfg.frame_w), int(rp.cfg.frame_h)
    assert rp.cfg.crop_x == 0 and w == rp.cfg.level_w[rp.cfg.levels - 1], "a whole-width frame: the star stage wraps in x"
    rp.set_uniforms(*T.uniforms(camera=cam, black_hole=bh, integration_method=1))
    per = _samples(rp, cam, StillCamera.equirect(), Observer(VEL), n)
    starred, lit = [], []
    for r, rec, beam in per:
        t, add, _ = AS.starred(r.reshape(h, w, 4), cat, None, sky, True)         # over the UNBEAMED results: static-frame escape directions
        starred.append(_beamed(t.reshape(-1, 4), rec, beam, sky))
        lit.append(add[..., 3] > 0)
    want = A.mean(A.accumulate(starred, sky))
    seam = [int(m[:, [0, w - 1]].sum()) for m in lit]
    print("lit pixels per sample:", [int(m.sum()) for m in lit], "in the first and last column:", seam)
    assert all(m.sum() >= 10 for m in lit) and all(v >= 1 for v in seam)
    rp.accum_set_camera(StillCamera.equirect())
    rp.set_stars(cat)
    rp.accum_set_stars(True)
    rp.accum_set_observer(VEL)
    got = _accumulate(rp, [n])
    _assert_words(got, want, "equirect, stars, beamed")
    # the starred pixels are beamed: beaming off differs on them
    rp.accum_set_observer(VEL, False)
    off = _accumulate(rp, [n])
    assert (_bits(off) != _bits(got)).any(axis=-1)[lit[0] | lit[1]].any(), "the starred pixels must carry the beam"
    unstarred = A.mean(A.accumulate([_beamed(r, rec, beam, sky) for r, rec, beam in per], sky))
    assert not np.array_equal(_bits(unstarred), _bits(want))
    rp.close()


# ---- 5. adaptive --------------------------------------------------------------------------------------------------
def test_adaptive_stills_see_the_beamed_samples():
    p = AR.Params(2, 6, 2, 0.05, 0.01)
    cam, still, sky = NEAR, StillCamera.equirect(), T.textures()[2]
    rp = _ctx(CFGS["37x33"]())
    rp.set_uniforms(*T.uniforms(camera=cam, integration_method=1))
    per = _samples(rp, cam, still, Observer(VEL), p.max_samples)
    beamed = [_beamed(r, rec, beam, sky) for r, rec, beam in per]
    st = AR.State(_npix(rp.cfg))
    info, actives = AR.call(st, p, beamed, sky)
    assert len(actives) >= 1 and len(np.unique(st.issued)) >= 2, "the scene must leave pixels at differing sample counts"
    rp.accum_set_camera(still)
    rp.accum_set_observer(VEL)
    rp.accum_begin()
    # each round's selection: the first call stops at min_samples, then one round at a time
    rp.accum_add_adaptive(p.min_samples, p.min_samples, p.round_samples, p.tolerance, p.dark)
    for k, want_active in enumerate(actives):
        got_active = np.sort(rp.accum_active_pixels(p.min_samples, p.max_samples, p.round_samples, p.tolerance, p.dark))
        assert np.array_equal(got_active, want_active), f"the selection of round {k + 1}"
        rp.accum_add_adaptive(p.min_samples, p.min_samples + (k + 1) * p.round_samples, p.round_samples, p.tolerance, p.dark)
    assert np.array_equal(rp.accum_read_counts().reshape(-1), st.issued)
    _assert_words(rp.accum_read(), AR.mean(st), "the adaptive mean, round by round")
    rp.accum_set_launch_rays(_npix(rp.cfg) // 3)                  # the rounds cut into several launches, one call: the same words, the same report
    rp.accum_begin()
    assert rp.accum_add_adaptive(**p.as_kwargs()) == info
    assert np.array_equal(rp.accum_read_counts().reshape(-1), st.issued)
    _assert_words(rp.accum_read(), AR.mean(st), "the adaptive mean, one call")
    rp.close()


# ---- 6. lensed meshes -----------------------------------------------------------------------------------------------
def test_a_lensed_mesh_in_a_still_under_an_observer():
    n = 3
    sky = T.textures()[2]
    rp = GL._ctx(((48, 32),), tuple(GL.SCENES["front_beside_the_hole"][1]), lensed=False)
    rp.set_uniforms(*GL._uniforms(None, 1, 1))
    rp.set_mesh_lensing(B.LENS_FRAMES | B.LENS_RAYS)
    per = _samples(rp, B.Camera(), None, Observer(VEL2), n)      # trace_rays is lensed too
    want = A.mean(A.accumulate([_beamed(r, rec, beam, sky) for r, rec, beam in per], sky))
    rp.accum_set_observer(VEL2)
    got = _accumulate(rp, [n])
    _assert_words(got, want, "the lensed still")
    rp.set_mesh_lensing(0)
    assert int((_bits(_accumulate(rp, [n])) != _bits(got)).any(axis=-1).sum()) >= 1, "the still must show the lensed mesh"
    rp.close()


# ---- 7. off is off ------------------------------------------------------------------------------------------------
def test_an_observer_set_and_cleared_leaves_every_bit():
    never = _ctx()
    never.set_uniforms(*T.uniforms(camera=NEAR, integration_method=1))
    want = _accumulate(never, [3])
    never.render()
    frame = never.read_hdr().copy()
    rays = cameras.pinhole_rays(NEAR, 48, 32)
    batch = never.trace_rays(rays)
    never.close()
    rp = _ctx()
    rp.accum_set_observer(VEL)                                    # accepted before the uniforms and before begin
    rp.set_uniforms(*T.uniforms(camera=NEAR, integration_method=1))
    moving = _accumulate(rp, [3])
    assert not np.array_equal(_bits(moving), _bits(want))
    rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(frame)), "a frame changed under an observer"
    assert np.array_equal(_bits(rp.trace_rays(rays)), _bits(batch)), "a ray batch changed under an observer"
    rp.accum_set_observer(None)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want)), "cleared by NULL"
    rp.accum_set_observer(VEL)
    rp.accum_set_observer((0.0, 0.0, 0.0), beaming=True)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want)), "cleared by a zero velocity"
    rp.accum_set_observer((0.0, -0.0, 0.0), beaming=False)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(want))
    rp.accum_set_observer(VEL)
    assert np.array_equal(_bits(_accumulate(rp, [3])), _bits(moving))
    rp.close()


def test_a_refused_observer_leaves_the_one_in_force():
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=NEAR, integration_method=1))
    L, h = rp._L, rp._h
    for in_force in (Observer(VEL2), None):
        rp.accum_set_observer(in_force)
        rays = rp.accum_sample_rays(1)

        def bad(velocity=(0.1, 0.0, 0.0), **kw):
            s = Observer(velocity).struct()
            for k, v in kw.items():
                setattr(s, k, v)
            rc = L.bhray_accum_set_observer(h, C.byref(s))
            if rc != 0:
                assert L.bhray_last_error(h), "a refusal carries a message"
                assert np.array_equal(_bits(rp.accum_sample_rays(1)), _bits(rays)), f"a refused observer changed the state: {velocity} {kw}"
            return rc
        assert bad(struct_size=16) == E_INVALID and bad(struct_size=24) == E_INVALID
        for v in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, -float("inf"))):
            assert bad(v) == E_INVALID, v
        assert bad((0.995, 0.0, 0.0)) == E_INVALID and bad((0.7, 0.7, 0.1)) == E_INVALID
        assert bad(beaming=2) == E_INVALID
        assert bad((0.0, 0.0, 0.0), beaming=2) == E_INVALID, "beaming is checked whatever the velocity"
    assert L.bhray_accum_set_observer(None, None) == E_INVALID
    rp.close()


# ---- 8. oracle ------------------------------------------------------------------------------------------------------
def test_the_still_against_the_oracle():
    n, vel = 2, (0.4, 0.0, 0.2)
    cfg = B.ladder_from_base((24, 16), 3, 1)
    u = T.uniforms(camera=NEAR, integration_method=1)
    sc = T.oracle_scene(*u, T.textures())
    sky = T.textures()[2]
    from tests import still_camera_ref as SR
    per = []
    for s in range(n):
        rec, beam = OR.sample_rays(NEAR.uniform(), cfg, SR.Still(SR.EQUIRECT), vel, s)
        res, _ = RR.oracle_rays(sc, rec)
        per.append(_beamed(res, rec, beam, sky))
    assert all(np.isfinite(r).all() for r in per)
    want = A.mean(A.accumulate(per, sky))
    rp = _ctx(cfg)
    rp.set_uniforms(*u)
    rp.accum_set_camera(StillCamera.equirect())
    rp.accum_set_observer(vel)
    got = _accumulate(rp, [n]).reshape(-1, 4)
    assert np.array_equal(got[:, 3], want[:, 3])
    bar = 2 * T.REL_TOL + (n + 1) * 2.0 ** -23                    # tests/test_gpu_still_camera.py's bar for colours
    err = float(T.rel_err(got[:, 0:3], want[:, 0:3]).max())
    print(f"max rel err {err:.3g} (bar {bar:.3g}); bit-identical {100.0 * float((_bits(got) == _bits(want)).all(axis=1).mean()):.2f} %")
    assert err <= bar, f"max rel err {err:.3g} > {bar:.3g}"
    rp.close()


# ---- 9. physics -----------------------------------------------------------------------------------------------------
def test_moving_towards_the_hole_shrinks_it():
    bh = B.BlackHole(accretion_disk_rotation=(float(np.pi / 2), 0.0, 0.0))
    normal = np.frombuffer(bh.uniform(), np.float32)[8:11]
    assert abs(abs(float(normal[2])) - 1.0) <= 1e-6, f"the disk's axis must be the z axis: {normal}"
    cam = B.Camera()                                              # (0, 0, -19) looking along +z: on the axis, at the hole's centre
    r = B.Renderer(CFGS["48x32"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.camera, r.black_hole = cam, bh
    r.ray_details.integration_method = 1
    rest = cameras.pinhole_rays(cam, 48, 32)
    counts = []
    for beta in (-0.5, 0.0, 0.5):
        rays, _ = cameras.boost_rays(rest, Observer((0.0, 0.0, beta)))
        rec = r.render_records(rays, (32, 48))
        counts.append(int(((rec["hit"] & 0xFF) == B.HIT_HORIZON).sum()))
    print("first hits on the horizon at beta = -0.5, 0, +0.5 along forward:", counts)
    assert counts[0] > counts[1] > counts[2] > 0, counts
    r.ray_pass.close()


# ---- 10. display, 11. Renderer, 12. the program ---------------------------------------------------------------------
def test_the_display_read_under_an_observer():
    rp = _ctx()
    rp.set_uniforms(*T.uniforms(camera=NEAR, integration_method=1))
    rp.accum_set_observer(VEL)
    mean = _accumulate(rp, [4])
    disp = rp.accum_read_display()
    with np.errstate(over="ignore"):
        sky16 = mean.astype(np.float16)
    assert disp.shape == (32, 48, 4) and np.array_equal(disp, P.post_ref(sky16)), "the display read differs from post_ref over the binary16 mean"
    assert np.array_equal(_bits(rp.accum_read()), _bits(mean)), "the display read changed the mean"
    rp.close()


def test_render_still_takes_the_observer():
    r = B.Renderer(CFGS["48x32"](), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    r.camera = NEAR
    still = r.render_still(samples=4, camera=StillCamera.equirect(), observer=Observer(VEL2))
    rp = _ctx()
    rp.set_uniforms(r.camera.uniform(), r.black_hole.uniform(), r.ray_details.uniform())
    rp.accum_set_camera(StillCamera.equirect())
    rp.accum_set_observer(VEL2)
    assert np.array_equal(_bits(still), _bits(_accumulate(rp, [4])))
    unbeamed = r.render_still(samples=4, camera=StillCamera.equirect(), observer=Observer(VEL2, beaming=False))
    rp.accum_set_observer(Observer(VEL2, beaming=False))
    assert np.array_equal(_bits(unbeamed), _bits(_accumulate(rp, [4]))) and not np.array_equal(_bits(unbeamed), _bits(still))
    p = AR.Params(2, 6, 2, 0.05, 0.01)
    adaptive = r.render_still(adaptive=B.AdaptiveStill(**p.as_kwargs()), observer=Observer(VEL))
    rp.accum_set_camera(None)
    rp.accum_set_observer(VEL)
    rp.accum_begin()
    assert rp.accum_add_adaptive(**p.as_kwargs()) == r.still_info
    assert np.array_equal(_bits(adaptive), _bits(rp.accum_read()))
    plain = r.render_still(samples=4)                             # observer=None: at rest again
    rp.accum_set_observer(None)
    assert np.array_equal(_bits(plain), _bits(_accumulate(rp, [4])))
    r.ray_pass.close()
    rp.close()


def test_cpp_host_writes_a_still_with_the_observer(tmp_path):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    base = ["--rk", "--base", "48", "32", "--levels", "1", "--disk-size", "64", "--spp", "2"]
    images = {}
    for name, args in (("rest", []), ("moving", ["--observer", "0.5", "0", "0"]), ("unbeamed", ["--observer", "0.5", "0", "0", "--no-beaming"])):
        out = tmp_path / f"{name}.f32"
        r = subprocess.run([exe, str(out)] + base + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == "48x32"
        images[name] = np.fromfile(out, dtype=np.float32).reshape(32, 48, 4)
    assert not np.array_equal(_bits(images["moving"]), _bits(images["rest"])), "--observer must change the image"
    from bhusie_amd import assets
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)    # bhray_render's textures
    r2 = B.Renderer(CFGS["48x32"](), device=0)
    r2.ray_pass.set_textures(grey, assets.reference_disk_texture(64), grey)
    r2.ray_details.integration_method = 1
    assert np.array_equal(_bits(images["moving"]), _bits(r2.render_still(samples=2, observer=Observer((0.5, 0.0, 0.0))))), "the C++ host's still differs from the Python host's"
    assert np.array_equal(_bits(images["unbeamed"]), _bits(r2.render_still(samples=2, observer=Observer((0.5, 0.0, 0.0), beaming=False))))
    assert np.array_equal(_bits(images["rest"]), _bits(r2.render_still(samples=2)))
    r2.ray_pass.close()
