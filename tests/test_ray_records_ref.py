"""CPU: the NumPy restatement of the ray records (tests/ray_records_ref.py) is pinned to the two oracles it restates, and the ray lists of
tests/test_gpu_ray_records.py meet the conditions that make the GPU comparison mean something - all on the reference alone."""
import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import cameras
from oracle import np_ray as N
from oracle import oracle as O
from tests import common as T
from tests import ray_records_ref as R
from tests import rays_ref as RR

W, H = 96, 54
INSIDE = B.Camera(position=(3.0, -2.0, -8.0), forward=(-0.3, 0.2, 1.0), fov=1.3)      # §15's camera inside the sphere


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
def test_results_equal_np_ray_bit_for_bit_on_the_seeded_list(method):
    out, rec, margin, _ = R.seeded_reference(method)
    rays = RR.seeded_rays()
    want = N.trace_rays(R.np_scene(RR.scene_uniforms(method)), rays[:, 0:3].copy(), rays[:, 4:7].copy())
    assert np.array_equal(_bits(out), _bits(want))
    # the conditions of the GPU comparison, on the reference alone
    k = R.kinds(rec)
    low = int((margin < R.MARGIN_BAR).sum())
    print(k, f"{low} of {rays.shape[0]} rays with a break-test margin below {R.MARGIN_BAR}")
    assert rays.shape[0] == 4133 and min(k["none"], k["horizon"], k["disk"]) >= 300 and k["mesh"] == 0, k
    assert low <= R.MARGIN_SHARE * rays.shape[0], f"{low} rays sit on the break test's threshold"
    assert (rec["triangle"] == -1).all() and (rec["hit"] >> 8 == 0).all()
    assert ((rec["transmittance"] >= 0.0) & (rec["transmittance"] <= 1.0)).all() and (rec["iterations"] <= 2000).all()
    # a record agrees with its result: a ray that hit nothing and took more than 5 iterations escapes (alpha 0), every other ray is a colour
    escaped = ((rec["hit"] & 0xFF) == B.HIT_NONE) & (rec["iterations"] > 5)
    assert np.array_equal(out[:, 3] == 0.0, escaped)


def test_results_equal_np_ray_bit_for_bit_on_the_mesh_list_and_its_conditions():
    out, rec, margin, after_march = R.mesh_reference(1)
    rays = R.mesh_rays()
    arrays = [m.arrays() for m in R.mesh_models()]
    want = N.trace_rays(R.np_scene(R.mesh_uniforms(1), arrays), rays[:, 0:3].copy(), rays[:, 4:7].copy())
    assert np.array_equal(_bits(out), _bits(want))
    c = R.mesh_conditions(rec, after_march)
    print(c, R.kinds(rec))
    assert rays.shape[0] % 64 != 0 and 900 <= rays.shape[0] <= 1100
    assert c["mesh_slot0"] >= 150 and c["mesh_slot2"] >= 150, c
    assert c["after_march"] >= 50, c
    assert c["distinct_triangle_indices"] >= 30, c
    assert c["mesh_slot1"] == 0, "slot 1 is invisible"
    assert int((margin < R.MARGIN_BAR).sum()) <= R.MARGIN_SHARE * rays.shape[0]
    mesh = (rec["hit"] & 0xFF) == B.HIT_MESH
    assert (rec["triangle"][mesh] >= 0).all() and (rec["triangle"][mesh] < arrays[0]["triangles"].shape[0]).all() and (rec["triangle"][~mesh] == -1).all()


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("camera", ["default", "inside"])
def test_closest_and_iterations_equal_the_c_oracles_aux_channels(camera, method):
    cam = B.Camera() if camera == "default" else INSIDE
    u = T.uniforms(camera=cam, integration_method=method)
    aux = O.render_aux(T.oracle_scene(*u, T.textures()), (W, H))
    out, rec, _, _ = R.trace(u, cameras.pinhole_rays(cam, W, H))
    assert np.array_equal(_bits(rec["closest"].reshape(H, W)), _bits(aux[..., 0])), "closest approach differs from oracle.render_aux"
    assert np.array_equal(rec["iterations"].reshape(H, W).astype(np.float32), aux[..., 1]), "iterations differ from oracle.render_aux"
    assert len(np.unique(rec["hit"] & 0xFF)) >= 3, "the frame must show the horizon, the disk and the sky"
