"""-m gpu: the display pass (bloom, mix, ACES, FXAA into the RGBA8 sRGB image) held byte for byte to tests/post_ref.py,
the NumPy restatement of bloom_down / bloom_up / mix / hdr / fxaa.wgsl, applied to the sky image the same frame's sky pass produced."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets, layouts
from tests import common as T
from tests import post_ref as P

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -5

POSE_IN = B.Camera()                                                                    # (0, 0, -19): inside the relativity sphere (R = 20)
POSE_OUT = B.Camera(position=(3.0, 4.0, -34.0), forward=(-0.08, -0.1, 1.0), fov=1.1)   # outside it


def _rp(cfg, tex, camera=POSE_IN, method=1, model=None, **kw):
    rp = B.RayPass(cfg, device=0, **kw)
    rp.set_textures(*tex)
    if model is not None:
        rp.upload_model(model)
    rp.set_uniforms(*T.uniforms(camera=camera, integration_method=method, model_count=1 if model is not None else 0))
    return rp


def _fxaa_tuple(f):
    return (np.float32(f.edge_threshold_min), np.float32(f.edge_threshold_max), int(f.iterations), np.float32(f.subpixel_quality))


def _check(rp, fxaa=None, mix=None):
    rp.render()
    rp.resolve_display()
    got = rp.read_display()
    sky = rp.read_sky()
    df, dm = B.post_defaults()
    want = P.post_ref(sky, _fxaa_tuple(fxaa) if fxaa is not None else _fxaa_tuple(df), np.float32(mix if mix is not None else dm.mix_ratio))
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = (got != want).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:5].tolist()}"
    return got, sky


CONFIGS = {
    "256x256_one_level": lambda: B.ladder_from_base((256, 256), 3, 1),
    "1920x1080": lambda: B.ladder_for_frame((1920, 1080), 3, 4),
    "1918x1081_native": lambda: B.ladder_from_base((72, 41), 3, 4),
    "3840x2160": lambda: B.ladder_for_frame((3840, 2160), 3, 4),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_display_is_post_ref_of_the_sky_image_at_every_baseline_size(name):
    rp = _rp(CONFIGS[name](), T.textures())
    got, sky = _check(rp)
    assert len(np.unique(got[..., :3].reshape(-1, 3), axis=0)) > 50           # a real picture, not a flat frame
    assert (got[..., 3] == 255).all()
    rp.close()


def test_display_with_the_mesh_config(tmp_path):
    obj = tmp_path / "mesh.obj"
    obj.write_text(assets.icosphere_mesh_obj(5, radius=8.0, bump=0.15, seed=3))
    model = B.load_model(str(obj))
    rp = _rp(B.ladder_for_frame((1920, 1080), 3, 4), T.textures(), model=model)
    _check(rp)
    rp.close()


@pytest.mark.parametrize("method", [0, 1], ids=["euler", "rk"])
@pytest.mark.parametrize("pose", ["inside", "outside"])
def test_display_for_both_integrators_and_two_poses(method, pose):
    rp = _rp(B.ladder_from_base((72, 41), 3, 3), T.textures(), camera=POSE_IN if pose == "inside" else POSE_OUT, method=method)
    _check(rp)
    rp.close()


@pytest.mark.parametrize("fxaa,mix", [
    ((0.0833, 0.250, 12, 0.75), 0.7),        # Low / Low
    ((0.0078, 0.031, 12, 0.75), 0.7),        # Extreme / Extreme
    ((0.0078, 0.031, 1, 0.75), 0.7),         # no search loop
    ((0.0078, 0.031, 2, 0.75), 0.7),         # the loop's bound reached at once
    ((0.0078, 0.031, 6, 1.0), 0.7),          # QUALITY 1.0 and 1.5
    ((0.0078, 0.031, 20, 0.5), 0.7),         # every QUALITY case and the default
    ((0.0156, 0.063, 12, 0.75), 0.0),
    ((0.0156, 0.063, 12, 0.75), 1.0),
], ids=["low", "extreme", "it1", "it2", "it6", "it20", "mix0", "mix1"])
def test_post_uniforms(fxaa, mix):
    rp = _rp(B.ladder_from_base((72, 41), 3, 3), T.textures(), camera=POSE_OUT)
    f = layouts.BhrayFxaaDetails(*fxaa)
    rp.set_post_uniforms(f, mix)
    _check(rp, fxaa=f, mix=mix)
    rp.close()


def test_state_rules_and_async_tickets_in_order():
    cfg = B.ladder_from_base((72, 41), 3, 3)
    L = B.lib()
    rp = _rp(cfg, T.textures(), frames_in_flight=2)
    W, H = rp.frame_size
    buf = np.empty((H, W, 4), np.uint8)
    assert L.bhray_read_display(rp._h, buf.ctypes.data, W * 4) == E_STATE          # nothing rendered yet
    rp.render()
    assert L.bhray_read_display(rp._h, buf.ctypes.data, W * 4) == E_STATE          # read before resolve
    p, n = C.c_void_p(), C.c_size_t()
    assert L.bhray_display_device_ptr(rp._h, C.byref(p), C.byref(n)) == E_STATE
    rp.resolve_display()                                                           # implies the sky pass
    first = rp.read_display()
    sky_first = rp.read_sky()
    assert np.array_equal(first, P.post_ref(sky_first))
    assert L.bhray_read_display(rp._h, buf.ctypes.data, W * 4 - 1) == E_INVALID     # short pitch
    rp.set_uniforms(*T.uniforms(camera=POSE_OUT, integration_method=1, time=0.5))
    rp.render()                                                                    # a new frame makes the image stale
    assert L.bhray_read_display(rp._h, buf.ctypes.data, W * 4) == E_STATE
    f = layouts.BhrayFxaaDetails(0.0, 0.0, layouts.FXAA_MAX_ITERATIONS + 1, 0.75)
    assert L.bhray_set_post_uniforms(rp._h, bytes(f), bytes(layouts.BhrayMixDetails(0.7))) == E_INVALID
    # two slots in flight: every frame's ticket delivers that frame's own image, in order
    pinned = [B.PinnedFrame(H, W, rgba8=True) for _ in range(4)]
    tickets, skies = [], []
    for i in range(4):
        rp.set_uniforms(*T.uniforms(camera=POSE_IN if i % 2 else POSE_OUT, integration_method=i % 2, time=0.25 * i))
        rp.render()
        rp.resolve_display()
        pinned[i].array[...] = 7
        tickets.append(rp.read_display_async(pinned[i]))
        skies.append(rp.read_sky())
    assert tickets == sorted(tickets) and len(set(tickets)) == 4
    for i in range(4):
        rp.wait_read(tickets[i])
        assert np.array_equal(pinned[i].array, P.post_ref(skies[i])), i
    assert not np.array_equal(pinned[0].array, pinned[1].array)
    ptr, nbytes = rp.display_device_ptr()
    assert ptr and nbytes == W * H * 4
    for b in pinned:
        b.free()
    rp.close()


def test_small_frames_and_unwhole_frames_are_refused():
    tex = T.textures()
    rp = _rp(B.ladder_from_base((24, 14), 3, 2), tex)                              # 70 x 40: fine
    _check(rp)
    rp.close()
    rp = _rp(B.ladder_from_base((10, 30), 3, 2), tex)                              # 28 x 88: a bloom level would be empty
    rp.render()
    with pytest.raises(B.BhrayError) as e:
        rp.resolve_display()
    assert e.value.code == E_INVALID
    rp.close()
    cfg = B.ladder_from_base((72, 41), 3, 3)
    rp = _rp(cfg, tex, row_rank=0, row_world=2)                                    # BHRAY_GATHER_NONE: half the rows
    rp.render()
    with pytest.raises(B.BhrayError) as e:
        rp.resolve_display()
    assert e.value.code == E_STATE
    rp.close()


@pytest.mark.parametrize("gather_sky", [False, True], ids=["hdr_gather", "sky_gather"])
@pytest.mark.parametrize("layout", ["devices_0_0", "slabs_8"])
def test_multi_partition_ctx_gives_the_single_gpu_image(layout, gather_sky):
    cfg = B.ladder_from_base((72, 41), 3, 3)
    tex = T.textures()
    one = _rp(cfg, tex)
    want, _ = _check(one)
    one.close()
    H = int(cfg.frame_h)
    if layout == "devices_0_0":
        kw = dict(devices=[0, 0], stripe_rows=9)
    else:
        bounds = [round(H * i / 8) for i in range(9)]
        kw = dict(devices=[0] * 8, slab_row0=bounds)
    rp = B.RayPass(cfg, gather_sky=gather_sky, frames_in_flight=2, **kw)
    rp.set_textures(*tex)
    rp.set_uniforms(*T.uniforms(camera=POSE_IN, integration_method=1))
    rp.render()
    rp.resolve_display()
    assert np.array_equal(rp.read_display(), want)
    rp.render()                                                                   # stale again after the next frame
    with pytest.raises(B.BhrayError) as e:
        rp.read_display()
    assert e.value.code == E_STATE
    rp.resolve_display()
    buf = B.PinnedFrame(H, int(cfg.frame_w), rgba8=True)
    t = rp.read_display_async(buf)
    rp.wait_read(t)
    assert np.array_equal(buf.array, want)
    buf.free()
    rp.close()


def _cpp_frames(tmp_path, form, frames, pixel_bytes):
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    out = tmp_path / f"{form}.bin"
    r = subprocess.run([exe, "--handoff", form, str(frames), str(out), "--rk", "--base", "24", "14", "--levels", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    size, delivered = r.stdout.split()
    w, h = (int(v) for v in size.split("x"))
    assert int(delivered) == frames
    return np.fromfile(out, dtype=np.uint8).reshape(frames, h, w, pixel_bytes)


def test_cpp_host_display_handoff(tmp_path):
    """bhray_render --handoff display (Handoff::AsyncDisplay, 2 frames in flight): every delivered frame, in order, is post_ref of the
    sky image the same program's sky hand-off delivers for that frame."""
    n = 5
    disp = _cpp_frames(tmp_path, "display", n, 4)
    sky = _cpp_frames(tmp_path, "sky", n, 8).view(np.float16)
    for i in range(n):
        assert np.array_equal(disp[i], P.post_ref(sky[i])), i
    assert not np.array_equal(disp[0], disp[1])


def test_renderer_save_image_round_trips_through_pil(tmp_path):
    from PIL import Image
    r = B.Renderer(B.ladder_from_base((72, 41), 3, 3), device=0)
    r.ray_pass.set_textures(*T.textures())
    r.ray_details.integration_method = 1
    r.render(0.0)
    path = tmp_path / "frame.png"
    r.save_image(str(path))
    img = np.asarray(Image.open(path))
    disp = r.ray_pass.read_display()
    assert img.shape == disp.shape and (img[..., 3] == 255).all()
    assert np.array_equal(img[..., :3], disp[..., :3])
    r.ray_pass.close()
