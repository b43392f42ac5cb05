"""CPU: the moving observer of stills (bhray_accum_set_observer) without a device.

  1. bhray_observer_sample_rays_host - the kernels' own function compiled for the host - equals the NumPy restatement (tests/observer_ref.py) in every word of the
     records and of the beam, for the four cameras, both shapes and a cropped frame, s in {0, 1, 7} and four velocities; bhray_observer_boost_rays and
     cameras.boost_rays equal the same rule on the same rays.
  2. Against the binary64 formula: directions within 1e-5 per component, D within 1e-5 relative (five times the 2.1e-6 a binary32 evaluation in this order was
     measured at when the rule was chosen); the figures are printed.
  3. Closed forms: along and against beta the direction stays and D is the longitudinal Doppler factor; across beta, n . b^ = -beta.
  4. Boosting by beta and then by -beta returns n' within the same bar.
  5. No observer: NULL and a zero velocity are the still camera's records bit for bit, beam 1, whatever `beaming` says."""
import ctypes as C
import math

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras, layouts
from bhusie_amd.cameras import Observer, StillCamera
from tests import observer_ref as OR
from tests import still_camera_ref as SR

CFGS = {"48x32": lambda: B.ladder_from_base((48, 32), 3, 1), "37x33": lambda: B.ladder_from_base((37, 33), 3, 1), "40x36_cropped": lambda: B.ladder_for_frame((40, 36), 3, 2)}
CAM = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)
CAMERAS = {"pinhole": (StillCamera.pinhole(), SR.Still()),
           "equirect": (StillCamera.equirect(), SR.Still(SR.EQUIRECT)),
           "fisheye": (StillCamera.fisheye(3.4), SR.Still(SR.FISHEYE, fisheye_fov=3.4)),
           "lens": (StillCamera.pinhole(lens_radius=0.35, focus_distance=7.5), SR.Still(SR.PINHOLE, lens_radius=0.35, focus_distance=7.5))}
SAMPLES = (0, 1, 7)
BAR = 1e-5


def _basis():
    _, _, _, right, _, _, fwd_n = SR.frame_basis(CAM.uniform())
    return right, fwd_n


def along(axis, beta):
    """beta along the binary32 unit vector `axis`: float32(beta) * axis, each component then stepped towards zero while the library's bb exceeds
    BHRAY_OBSERVER_MAX_SPEED2 - at 0.99 the rounding of the products can carry bb a last bit past the limit, and the setter refuses that"""
    v = (np.float32(beta) * np.asarray(axis, dtype=np.float32)).astype(np.float32)
    for _ in range(8):
        if not OR.speed2(v) > OR.MAX_SPEED2:
            break
        v = np.nextafter(v, np.float32(0.0)).astype(np.float32)
    assert not OR.speed2(v) > OR.MAX_SPEED2
    return tuple(float(x) for x in v)


def velocities():
    right, fwd_n = _basis()
    return {"x_0.5": (0.5, 0.0, 0.0), "yz": (0.0, -0.3, 0.2), "forward_0.99": along(fwd_n, 0.99), "right_1e-4": along(right, 1e-4)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(cfg, cam_bytes, still, observer, s, want_beam=True):
    n = int(cfg.frame_w) * int(cfg.frame_h)
    out, beam = np.empty((n, 8), dtype=np.float32), np.empty(n, dtype=np.float32)
    st = still.struct() if still is not None else None
    ob = observer.struct() if observer is not None else None
    rc = B.lib().bhray_observer_sample_rays_host(C.byref(cfg), cam_bytes, C.byref(st) if st is not None else None, C.byref(ob) if ob is not None else None, int(s),
                                                 out.ctypes.data, beam.ctypes.data if want_beam else None)
    assert rc == 0, rc
    return out, beam


def lib_boost(rays, observer, want_beam=True):
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out, beam = np.empty_like(rays), np.empty(rays.shape[0], dtype=np.float32)
    ob = observer.struct() if observer is not None else None
    rc = B.lib().bhray_observer_boost_rays(C.byref(ob) if ob is not None else None, rays.ctypes.data, rays.shape[0], out.ctypes.data, beam.ctypes.data if want_beam else None)
    assert rc == 0, rc
    return out, beam


# ---- 1. the C text, the restatement and the package's function ------------------------------------------
@pytest.mark.parametrize("kind", list(CAMERAS))
@pytest.mark.parametrize("shape", list(CFGS))
def test_the_host_function_is_the_restatement(shape, kind):
    cfg = CFGS[shape]()
    still, ref = CAMERAS[kind]
    if shape == "40x36_cropped":
        assert (cfg.crop_x, cfg.crop_y) != (0, 0) or (cfg.frame_w, cfg.frame_h) != tuple(cfg.sizes()[-1]), "the frame must be a window of its level"
    for name, vel in velocities().items():
        assert float(OR.speed2(vel)) <= float(OR.MAX_SPEED2), name
        for s in SAMPLES:
            rest = SR.sample_rays(CAM.uniform(), cfg, ref, s)
            want, want_beam = OR.boost_rays(rest, vel)
            got, beam = host(cfg, CAM.uniform(), still, Observer(vel), s)
            differ = int((_bits(got) != _bits(want)).sum()) + int((_bits(beam) != _bits(want_beam)).sum())
            assert differ == 0, f"{kind} {name} sample {s}: {differ} words of the host function differ from the restatement"
            assert np.array_equal(_bits(host(cfg, CAM.uniform(), still, Observer(vel, beaming=False), s, want_beam=False)[0]), _bits(want)), "beaming and a NULL out_beam leave the records alone"
            got2, beam2 = lib_boost(rest, Observer(vel))
            differ = int((_bits(got2) != _bits(want)).sum()) + int((_bits(beam2) != _bits(want_beam)).sum())
            assert differ == 0, f"{kind} {name} sample {s}: {differ} words of bhray_observer_boost_rays differ from the restatement"
            mine, mine_beam = cameras.boost_rays(rest, Observer(vel))
            differ = int((_bits(mine) != _bits(want)).sum()) + int((_bits(mine_beam) != _bits(want_beam)).sum())
            assert differ == 0, f"{kind} {name} sample {s}: {differ} words of cameras.boost_rays differ from the restatement"
            assert np.array_equal(_bits(got[:, 0:4]), _bits(rest[:, 0:4])), "the origin is unchanged"
            if kind == "fisheye":
                dead = (rest[:, 4:7] == 0).all(axis=1)
                assert 0 < int(dead.sum()) < dead.size and np.array_equal(_bits(got[dead]), _bits(rest[dead])) and (beam[dead] == 1.0).all(), "outside the circle: unchanged, beam 1"


def test_boost_in_place_and_without_a_beam():
    cfg = CFGS["37x33"]()
    rest = SR.sample_rays(CAM.uniform(), cfg, SR.Still(SR.EQUIRECT), 1)
    ob = Observer((0.0, -0.3, 0.2)).struct()
    want, _ = OR.boost_rays(rest, (0.0, -0.3, 0.2))
    buf = rest.copy()
    assert B.lib().bhray_observer_boost_rays(C.byref(ob), buf.ctypes.data, buf.shape[0], buf.ctypes.data, None) == 0
    assert np.array_equal(_bits(buf), _bits(want))
    assert B.lib().bhray_observer_boost_rays(C.byref(ob), None, 0, None, None) == 0, "no rays: nothing to do"


# ---- 2. against the binary64 formula ----------------------------------------------------------------------
def test_the_rule_lies_on_the_binary64_formula():
    rng = np.random.default_rng(26)
    worst_n = worst_d = worst_len = 0.0
    for _ in range(40):
        n = rng.normal(size=(500, 3))
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        n = SR._unit(n)                                           # unit as a binary32 normalise leaves them: what still_record hands over
        b = rng.normal(size=3)
        b = b / np.linalg.norm(b) * rng.uniform(0.0, 0.9899)
        vel = tuple(float(v) for v in b.astype(np.float32))
        got, beam = OR.boost(n, vel)
        want, D = OR.exact(n, np.asarray(vel, dtype=np.float32))
        worst_n = max(worst_n, float(np.abs(got.astype(np.float64) - want / np.linalg.norm(want, axis=1, keepdims=True)).max()))
        worst_len = max(worst_len, float(np.abs(np.linalg.norm(want, axis=1) - 1.0).max()))
        worst_d = max(worst_d, float(np.abs(beam.astype(np.float64) ** 0.25 / D - 1.0).max()))
    print(f"20000 pairs, |beta| <= 0.99: worst component error {worst_n:.3g}, worst relative error of D {worst_d:.3g}, the formula's own length within {worst_len:.3g} of 1")
    assert worst_n <= BAR and worst_d <= BAR
    # ... and the records of a frame at the fastest velocity of the cases
    cfg = CFGS["48x32"]()
    for name, vel in velocities().items():
        rest = SR.sample_rays(CAM.uniform(), cfg, SR.Still(SR.EQUIRECT), 7)
        got, beam = OR.boost(rest[:, 4:7], vel)
        want, D = OR.exact(rest[:, 4:7], np.asarray(vel, dtype=np.float32))
        en = float(np.abs(got.astype(np.float64) - want).max())
        ed = float(np.abs(beam.astype(np.float64) ** 0.25 / D - 1.0).max())
        print(f"equirect 48x32 sample 7, {name}: component error {en:.3g}, relative error of D {ed:.3g}")
        assert en <= BAR and ed <= BAR, name


# ---- 3. closed forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [1e-4, 0.3, 0.5, 0.9, 0.99])
def test_closed_forms(beta):
    axis = np.array([0.6, 0.0, 0.8], dtype=np.float32)           # a unit vector exact in binary32
    across = np.array([0.8, 0.0, -0.6], dtype=np.float32)
    vel = along(axis, beta)
    b = float(np.sqrt(np.float64(OR.speed2(vel))))
    n, beam = OR.boost(np.stack([axis, -axis, across]), vel)
    D = beam.astype(np.float64) ** 0.25
    assert np.abs(n[0] - axis).max() <= BAR and abs(D[0] / math.sqrt((1 + b) / (1 - b)) - 1) <= BAR, "looking along beta"
    assert np.abs(n[1] + axis).max() <= BAR and abs(D[1] / math.sqrt((1 - b) / (1 + b)) - 1) <= BAR, "looking against beta"
    assert abs(float(n[2].astype(np.float64) @ axis.astype(np.float64)) + b) <= BAR, "looking across beta: n . b^ = -beta"
    got, _ = lib_boost(np.concatenate([np.zeros((3, 4), np.float32), np.stack([axis, -axis, across]), np.zeros((3, 1), np.float32)], axis=1), Observer(vel))
    assert np.array_equal(_bits(got[:, 4:7]), _bits(n))


def test_the_issues_numbers():
    """beta = 0.5: a direction 90 degrees off the velocity is displaced by 30 degrees; the sky ahead brightens by 9 and the sky behind dims to a ninth"""
    n, beam = OR.boost(np.array([[0, 1, 0], [1, 0, 0], [-1, 0, 0]], dtype=np.float32), (0.5, 0.0, 0.0))
    assert abs(math.degrees(math.asin(-float(n[0, 0]))) - 30.0) <= 1e-3
    assert abs(float(beam[1]) - 9.0) <= 9.0 * 4 * BAR and abs(float(beam[2]) - 1.0 / 9.0) <= 4 * BAR / 9.0


# ---- 4. the inverse -------------------------------------------------------------------------------------------
def test_boosting_back_returns_the_direction():
    cfg = CFGS["37x33"]()
    rest = SR.sample_rays(CAM.uniform(), cfg, SR.Still(SR.EQUIRECT), 1)[:, 4:7]
    worst = 0.0
    for name, vel in velocities().items():
        n, _ = OR.boost(rest, vel)
        back, _ = OR.boost(n, tuple(-v for v in vel))
        err = float(np.abs(back.astype(np.float64) - rest).max())
        print(f"{name}: beta then -beta returns n' within {err:.3g}")
        worst = max(worst, err)
        assert err <= BAR, name


# ---- 5. no observer -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(CAMERAS))
def test_a_zero_velocity_is_no_observer(kind):
    cfg = CFGS["37x33"]()
    still, ref = CAMERAS[kind]
    for s in SAMPLES:
        want = SR.sample_rays(CAM.uniform(), cfg, ref, s)
        for ob in (None, Observer(), Observer((0.0, 0.0, 0.0), beaming=False), Observer((0.0, -0.0, 0.0))):
            got, beam = host(cfg, CAM.uniform(), still, ob, s)
            assert np.array_equal(_bits(got), _bits(want)) and (beam == 1.0).all(), (kind, s, ob)
            got, beam = lib_boost(want, ob)
            assert np.array_equal(_bits(got), _bits(want)) and (beam == 1.0).all()
            got, beam = cameras.boost_rays(want, ob)
            assert np.array_equal(_bits(got), _bits(want)) and (beam == 1.0).all()
    d = layouts.BhrayObserver()
    B.lib().bhray_observer_default(C.byref(d))
    assert (d.struct_size, tuple(d.velocity), d.beaming) == (20, (0.0, 0.0, 0.0), 1) and Observer().at_rest
