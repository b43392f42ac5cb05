"""-m gpu: the display kernels at the smallest and oddest legal frames, and one frame held to the reference's EXECUTED shader text with no
restatement anywhere in the chain.  Reads only tests/golden/.

  * Small and odd frames: one-level ctxs at 32x32 (the deepest bloom level is one texel), 33x32, 32x47, 63x35 (levels of odd width 31, 15,
    7, 3, 1) and 131x70 (wider than one 64-pixel row of threads, a multiple of nothing), the adaptive-RK camera inside and outside the
    relativity sphere: `resolve_display` equals tests/post_ref.py of the device's own `read_sky`, byte for byte (the `_check` of
    tests/test_gpu_display.py; post_ref.py itself is held word for word to the executed shaders by tests/test_wgsl_post_pin.py).  31x32 and 32x31
    are refused with BHRAY_E_INVALID.
  * Direct leg: `direct45` of tests/golden/wgsl_exec_post.npz is a scene whose frame - ray.wgsl executed by oracle/wgsl_exec.py - holds only
    direction pixels and the horizon's constant (0, 0, 0, 1): the disk lies inside the unit horizon sphere, the camera inside the
    relativity sphere.  Those are the pixels the BHRAY_F_LITERAL kernel reproduces in every word (tests/test_gpu_literal.py; colours would
    go through the device's pow), so the literal ctx's `read_hdr` and `read_sky` must equal the fixture's frame and sky image in every word,
    and `read_display` then equals the RGBA8 bytes that the executed bloom / mix / hdr / fxaa shaders gave for that sky image.
"""
import os

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T
from tests import test_gpu_display as D

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("pose", ["inside", "outside"])
@pytest.mark.parametrize("size", [(32, 32), (33, 32), (32, 47), (63, 35), (131, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_odd_frames_are_post_ref_of_their_own_sky_image(size, pose):
    cfg = B.ladder_from_base(size, 3, 1)
    assert (int(cfg.frame_w), int(cfg.frame_h)) == size
    rp = D._rp(cfg, T.textures(), camera=D.POSE_IN if pose == "inside" else D.POSE_OUT, method=1)
    got, sky = D._check(rp)
    assert got.shape == (size[1], size[0], 4) and B.bloom_sizes(*size)[4] == (size[0] // 32, size[1] // 32)
    assert len(np.unique(got[..., :3].reshape(-1, 3), axis=0)) > 20            # a picture, not a flat frame
    rp.close()


@pytest.mark.parametrize("size", [(31, 32), (32, 31)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_one_pixel_under_the_minimum_are_refused(size):
    rp = D._rp(B.ladder_from_base(size, 3, 1), T.textures())
    rp.render()
    with pytest.raises(B.BhrayError) as e:
        rp.resolve_display()
    assert e.value.code == D.E_INVALID
    rp.close()


def test_direct_leg_literal_frame_sky_and_display_equal_the_executed_shaders():
    g = np.load(os.path.join(GOLD, "wgsl_exec_post.npz"))
    r = np.load(os.path.join(GOLD, "wgsl_exec.npz"))
    size = tuple(int(v) for v in g["direct45.size"])
    rp = B.RayPass(B.ladder_from_base(size, 3, 1), device=0, literal=True)
    rp.set_textures(r["t_temp"], r["t_disk"], r["t_sky"])
    rp.set_uniforms(g["direct45.camera"].tobytes(), g["direct45.black_hole"].tobytes(), g["direct45.details"].tobytes())
    assert g["direct45.fxaa_details"].tobytes() == bytes(B.post_defaults()[0]) and g["direct45.mix_details"].tobytes() == bytes(B.post_defaults()[1])
    rp.render()
    frame, want = rp.read_hdr(), g["direct45.frame"]
    bad = (frame.view(np.uint32) != want.view(np.uint32)).any(axis=-1)
    assert not bad.any(), f"ray frame: {int(bad.sum())} pixels differ from the executed ray.wgsl, first at (y, x) {np.argwhere(bad)[:5].tolist()}"
    rp.resolve_display()
    sky, want = rp.read_sky().view(np.uint16), g["direct45.sky"]
    bad = (sky != want).any(axis=-1)
    assert not bad.any(), f"sky image: {int(bad.sum())} pixels differ from the executed sky.wgsl, first at (y, x) {np.argwhere(bad)[:5].tolist()}"
    got, want = rp.read_display(), g["direct45.rgba8"]
    bad = (got != want).any(axis=-1)
    assert not bad.any(), f"display: {int(bad.sum())} pixels differ from the executed display shaders, first at (y, x) {np.argwhere(bad)[:5].tolist()}"
    assert len(np.unique(got[..., :3].reshape(-1, 3), axis=0)) > 50 and (got[..., 3] == 255).all()
    rp.close()
