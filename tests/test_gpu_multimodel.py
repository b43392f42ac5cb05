"""-m gpu: scenes with several models (BHRAY_MAX_MODELS = 8): ray.wgsl:377-389's loop over model_count with MAX_MODELS raised.

Slots 0 .. model_count-1 are traced in index order, an invisible slot, one never uploaded and one uploaded with 0 triangles are
skipped, the strictly nearer hit wins (a tie keeps the lower index) and the diffuse factor is the winner's.  Every case runs with the
latency build and with the build for a saturated device (BHRAY_TRACE_DENSE=0/1): the second traverses the models inside the parked
region of its flat phase.  Every mesh stands outside the relativity sphere (radius 20): the shader tests meshes in flat space only.
"""
import os
import subprocess

import numpy as np
import pytest

import bhusie_amd as B
from bhusie_amd import assets
from oracle import oracle as O
from tests import common as T
from tests import post_ref as PR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CAM = B.Camera(position=(0.0, 0.0, -90.0), forward=(0.0, 0.0, 1.0), fov=0.7)
A, A2, BB, CC = (-30.0, 0.0, 0.0), (-27.0, 1.0, -3.0), (30.0, 2.0, 5.0), (0.0, -28.0, 0.0)
FRONT = (0.0, 8.0, -55.0)                  # 35 units in front of the camera: a slot that must NOT be drawn covers much of the frame
EMPTY = "empty"                            # a slot uploaded with a model of 0 triangles
# name: (model_count, {slot: (seed | EMPTY, position, visible)}); slots at or above model_count are uploaded and must not count
SCENES = {
    "two_overlapping": (2, {0: (3, A, 1), 1: (5, A2, 1)}),
    "three_with_holes": (3, {0: (7, BB, 1), 1: (5, A2, 0), 3: (3, FRONT, 1), 7: (9, FRONT, 1)}),        # invisible, never uploaded, above
    "eight": (8, {0: (3, A, 1), 1: (5, A2, 1), 2: (7, BB, 1), 3: (9, CC, 1), 4: (11, (0.0, 30.0, 10.0), 1), 5: (13, (-25.0, -25.0, 0.0), 0),
                  6: (EMPTY, (0.0, 0.0, 0.0), 1), 7: (15, (28.0, -22.0, -6.0), 1)}),
}


@pytest.fixture(params=["0", "1"], ids=["latency", "dense"])
def build(request, monkeypatch):
    monkeypatch.setenv("BHRAY_TRACE_DENSE", request.param)
    return request.param


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("meshes")


def _model(mesh_dir, seed, pos, vis, n_lat=14, n_lon=18, radius=12.0):
    if seed == EMPTY:
        m = B.Model()
    else:
        p = mesh_dir / f"s{seed}_{n_lat}_{n_lon}_{radius}.obj"
        if not p.exists():
            p.write_text(assets.sphere_mesh_obj(n_lat, n_lon, radius=radius, bump=0.2, seed=int(seed), with_normals=True))
        m = B.load_model(str(p))
    m.set_transform(pos, vis)
    return m


def _placeholder():
    """A slot the oracle must skip: a default ModelUniform (visible 0, no triangles: triangle.rs:297)."""
    return dict(position=(0.0, 0.0, 0.0), visible=0, points=np.zeros((0, 4), np.float32), normals=np.zeros((0, 4), np.float32),
                triangles=np.zeros((0, 6), np.int32), nodes=np.zeros(32, np.uint8), bvh_lookup=np.zeros(0, np.int32))


def _slots(mesh_dir, spec):
    return {i: _model(mesh_dir, *s) for i, s in spec.items()}


def _oracle_models(models, count):
    out = []
    for i in range(count):
        m = models.get(i)
        a = m.arrays() if m is not None else None
        out.append(a if a is not None and a["triangles"].shape[0] > 0 else _placeholder())
    return out


def _gpu(cfg, u, tex, models, **kw):
    rp = B.RayPass(cfg, device=0, **kw)
    rp.set_textures(*tex)
    for i, m in models.items():
        rp.upload_model(m, i)
    rp.set_uniforms(*u)
    rp.render()
    return rp


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("method", [1, 0])
@pytest.mark.parametrize("scene", list(SCENES))
def test_models_match_the_oracle(build, mesh_dir, scene, method):
    tex = T.textures()
    count, spec = SCENES[scene]
    models = _slots(mesh_dir, spec)
    u = T.uniforms(camera=CAM, integration_method=method, model_count=count)
    cfg = B.ladder_from_base((24, 14), 3, 3)                   # 24x14 -> 70x40 -> 208x118
    cnt = O.Counters()
    want = O.render_ladder(T.oracle_scene(*u, tex, _oracle_models(models, count)), cfg.sizes(), cnt)
    rp = _gpu(cfg, u, tex, models)
    for l in range(3):
        got = rp.read_level(l)
        T.assert_parity(got, want[l], f"{scene} method {method} level {l}")
        d = want[l][..., 3] == 0
        assert np.array_equal(_bits(got[d]), _bits(want[l][d])), f"{scene} level {l}: direction pixels must be bit-identical"
    rp.close()
    rc = _gpu(cfg, u, tex, models, counters=True)
    c = rc.counters()
    assert c == cnt.as_dict()
    assert c["triangles"] > 0 and c["node_pairs"] > 0
    T.assert_parity(rc.read_hdr(), want[-1], f"{scene} counting build")
    rc.close()
    bare = O.render_ladder(T.oracle_scene(*T.uniforms(camera=CAM, integration_method=method, model_count=0), tex), cfg.sizes())[-1]
    assert int((bare != want[-1]).any(axis=-1).sum()) > 100                                   # the models are in the picture


def _fixture_models(g, name, mesh_dir):
    n_lat, n_lon = (int(v) for v in g["mesh_params"])
    radius, bump = (float(v) for v in g["mesh_shape"])
    assert bump == 0.2
    out = {}
    for i, (seed, pos, vis) in enumerate(zip(g[f"{name}.seeds"], g[f"{name}.positions"], g[f"{name}.visible"])):
        if int(seed) >= 0:
            out[i] = _model(mesh_dir, int(seed), tuple(float(v) for v in pos), int(vis), n_lat, n_lon, radius)
    return out


@pytest.mark.parametrize("name", ["rk_pair", "euler_four", "rk_holes", "euler_three"])
def test_literal_kernel_reproduces_the_executed_shader(build, mesh_dir, name):
    """tests/golden/multimodel.npz: the reference's ray.wgsl executed with several models (tests/golden/make_golden_multimodel.py).  The
    literal kernel: every NaN pixel and class identical, direction pixels bit for bit, colours within the device-pow tolerance, mesh
    pixels bit for bit."""
    g = np.load(os.path.join(GOLD, "multimodel.npz"))
    tex = (g["t_temp"], g["t_disk"], g["t_sky"])
    u = tuple(g[f"{name}.{k}"].tobytes() for k in ("camera", "black_hole", "details"))
    sizes = [tuple(int(v) for v in s) for s in g[f"{name}.sizes"]]
    cfg = B.ladder_from_base(sizes[0], 3, len(sizes))
    assert cfg.sizes() == sizes
    rp = _gpu(cfg, u, tex, _fixture_models(g, name, mesh_dir), literal=True)
    for l in range(len(sizes)):
        got, want = rp.read_level(l), g[f"{name}.level{l}"]
        assert np.array_equal(got[..., 3], want[..., 3]), f"{name} level {l}: pixel classes"
        d = want[..., 3] == 0
        assert np.array_equal(_bits(got[d]), _bits(want[d])), f"{name} level {l}: direction pixels"
        e = np.abs(got - want) / np.maximum(np.abs(want), T.ABS_FLOOR)
        assert float(e.max(initial=0.0)) <= 1e-4, f"{name} level {l}: colour max rel {float(e.max())}"
    rp.close()


def test_a_duplicate_of_model_0_at_the_same_pose_changes_no_byte(build, mesh_dir):
    """Equal t on both models: the strictly-nearer rule keeps model 0's hit, and its shading is model 0's."""
    tex = T.textures()
    cfg = B.ladder_from_base((24, 14), 3, 3)
    for method in (1, 0):
        one = _gpu(cfg, T.uniforms(camera=CAM, integration_method=method, model_count=1), tex, {0: _model(mesh_dir, 3, A, 1)})
        two = _gpu(cfg, T.uniforms(camera=CAM, integration_method=method, model_count=2), tex, {0: _model(mesh_dir, 3, A, 1), 1: _model(mesh_dir, 3, A, 1)})
        assert np.array_equal(_bits(one.read_hdr()), _bits(two.read_hdr())), method
        one.close(); two.close()


def test_index_order_of_models_that_do_not_overlap_changes_no_byte(build, mesh_dir):
    tex = T.textures()
    cfg = B.ladder_from_base((24, 14), 3, 3)
    u = T.uniforms(camera=CAM, integration_method=1, model_count=3)
    spec = [(3, A, 1), (7, BB, 1), (9, CC, 1)]
    a = _gpu(cfg, u, tex, {i: _model(mesh_dir, *s) for i, s in enumerate(spec)})
    b = _gpu(cfg, u, tex, {i: _model(mesh_dir, *s) for i, s in enumerate(reversed(spec))})
    assert np.array_equal(_bits(a.read_hdr()), _bits(b.read_hdr()))
    a.close(); b.close()


def test_invisible_models_give_the_no_mesh_frame(build, mesh_dir):
    tex = T.textures()
    cfg = B.ladder_from_base((24, 14), 3, 3)
    bare = _gpu(cfg, T.uniforms(camera=CAM, integration_method=1, model_count=0), tex, {})
    models = {i: _model(mesh_dir, 3 + 2 * i, p, 0) for i, p in enumerate((A, BB, CC, FRONT))}
    rp = _gpu(cfg, T.uniforms(camera=CAM, integration_method=1, model_count=4), tex, models)
    assert np.array_equal(_bits(rp.read_hdr()), _bits(bare.read_hdr()))
    rp.set_model_transform(FRONT, 1, index=3)                  # and one of them made visible is drawn
    rp.render()
    assert not np.array_equal(_bits(rp.read_hdr()), _bits(bare.read_hdr()))
    rp.close(); bare.close()


def _moves():
    # (per-slot (position, visible) changes of this frame, integrator)
    return [({}, 1), ({1: (BB, 1)}, 1), ({0: (A2, 0)}, 1), ({2: (FRONT, 1), 0: (A, 1)}, 0), ({2: (CC, 0), 1: (A2, 1)}, 1),
            ({0: (A, 0), 1: (A2, 0)}, 1), ({3: ((0.0, 30.0, 10.0), 1)}, 1)]


def _frames(mesh_dir, cfg, tex, bind=False, **kw):
    spec = {0: (3, A, 1), 1: (5, A2, 1), 2: (7, CC, 1), 3: (9, BB, 0)}
    rp = B.RayPass(cfg, **kw)
    rp.set_textures(*tex)
    for i, s in spec.items():
        rp.upload_model(_model(mesh_dir, *s), i)
    out, bufs = [], []
    w, h = cfg.frame_w, cfg.frame_h
    for k, (moves, method) in enumerate(_moves()):
        for i, (pos, vis) in moves.items():
            rp.set_model_transform(pos, vis, index=i)
        rp.set_uniforms(*T.uniforms(camera=CAM, integration_method=method, model_count=4, time=0.1 * k))
        if bind:
            bufs.append(T.DeviceBuffer(w * h * 16))
            rp.bind_output(bufs[-1].ptr.value, bufs[-1].nbytes)
            rp.render()
        else:
            rp.render()
            out.append(rp.read_hdr().copy())
    if bind:
        rp.sync()
        for b in bufs:
            out.append(b.read(np.uint32))
            b.free()
    rp.close()
    return [o.view(np.uint32).ravel() for o in out]


def test_per_index_transforms_travel_with_their_frame(build, mesh_dir):
    """Transforms of several slots changed between frames, all frames enqueued back to back (several frame slots, batches, the issue threads
    of a multi-partition ctx), every frame against a one-slot ctx; the speculative, superset and temporal modes deliver the same frames."""
    tex = T.textures()
    cfg = B.ladder_for_frame((200, 110), 3, 3)
    want = _frames(mesh_dir, cfg, tex, device=0, frames_in_flight=1)
    assert len({w.tobytes() for w in want}) == len(want)                                   # every change is in the picture
    for kw in (dict(device=0, frames_in_flight=4, frames_per_batch=2), dict(devices=[0] * 3, stripe_rows=9, frames_in_flight=2),
               dict(device=0, frames_in_flight=2, speculative_levels=2), dict(device=0, superset_levels=2, frames_in_flight=2)):
        got = _frames(mesh_dir, cfg, tex, bind=True, **kw)
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (kw, k)
    got = _frames(mesh_dir, cfg, tex, device=0, temporal=True, frames_in_flight=1)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), ("temporal", k)


def test_eight_partitions_on_one_device_gather_the_undivided_frame(build, mesh_dir):
    tex = T.textures()
    count, spec = SCENES["eight"]
    u = T.uniforms(camera=CAM, integration_method=1, model_count=count)
    cfg = B.ladder_for_frame((320, 180), 3, 3)
    one = _gpu(cfg, u, tex, _slots(mesh_dir, spec), frames_in_flight=1)
    want = one.read_hdr()
    one.close()
    rp = B.RayPass(cfg, devices=[0] * 8, stripe_rows=9, frames_per_batch=2, frames_in_flight=2)
    rp.set_textures(*tex)
    for i, m in _slots(mesh_dir, spec).items():
        rp.upload_model(m, i)
    rp.set_uniforms(*u)
    for _ in range(3):
        rp.render()
    assert np.array_equal(_bits(rp.read_hdr()), _bits(want))
    rp.close()


def test_display_pass_of_a_multi_model_frame(build, mesh_dir):
    tex = T.textures()
    count, spec = SCENES["two_overlapping"]
    cfg = B.ladder_for_frame((200, 110), 3, 3)
    rp = _gpu(cfg, T.uniforms(camera=CAM, integration_method=1, model_count=count), tex, _slots(mesh_dir, spec))
    rp.resolve_display()
    got, sky = rp.read_display(), rp.read_sky()
    f, m = B.post_defaults()
    want = PR.post_ref(sky, (np.float32(f.edge_threshold_min), np.float32(f.edge_threshold_max), int(f.iterations), np.float32(f.subpixel_quality)),
                       np.float32(m.mix_ratio))
    assert np.array_equal(got, want)
    rp.close()


def test_cpp_host_with_two_obj_files(build, tmp_path):
    """bhray_render --obj a.obj --obj b.obj: the Renderer's add_model puts them in slots 0 and 1 (model_count 2); the same frame as the
    Python Renderer with two add_model calls."""
    exe = os.path.join(os.path.dirname(B.LIB_PATH), "bhray_render")
    objs = []
    for k, (seed, shift) in enumerate(((3, (-40.0, 10.0, 60.0)), (5, (30.0, -5.0, 70.0)))):   # OBJ units (load_model scales by (0.5, -0.5, 0.5))
        text = assets.sphere_mesh_obj(10, 12, radius=16.0, bump=0.2, seed=seed, with_normals=True)
        lines = []
        for ln in text.splitlines():
            if ln.startswith("v "):
                x, y, z = (float(v) for v in ln.split()[1:4])
                ln = "v %.6f %.6f %.6f" % (x + shift[0], y + shift[1], z + shift[2])
            lines.append(ln)
        p = tmp_path / f"m{k}.obj"
        p.write_text("\n".join(lines) + "\n")
        objs.append(p)
    out = tmp_path / "o.f32"
    r = subprocess.run([exe, str(out), "--rk", "--base", "24", "14", "--levels", "3", "--disk-size", "64", "--obj", str(objs[0]), "--obj", str(objs[1])],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w, h = (int(v) for v in r.stdout.strip().splitlines()[-1].split("x"))
    got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
    grey = np.full((1, 1, 4), (160, 160, 160, 255), np.uint8)                                # bhray_render's textures
    disk = assets.reference_disk_texture(64)
    r2 = B.Renderer(B.ladder_from_base((24, 14), 3, 3), device=0)
    r2.ray_pass.set_textures(grey, disk, grey)
    assert r2.add_model(B.load_model(str(objs[0]))) == 0 and r2.add_model(B.load_model(str(objs[1]))) == 1
    assert r2.ray_details.model_count == 2
    r2.ray_details.integration_method = 1
    r2.render()
    want = r2.read_hdr()
    assert np.array_equal(_bits(got), _bits(want))
    one = B.Renderer(B.ladder_from_base((24, 14), 3, 3), device=0)
    one.ray_pass.set_textures(grey, disk, grey)
    one.set_model(B.load_model(str(objs[0])))
    one.ray_details.integration_method = 1
    one.render()
    assert not np.array_equal(_bits(one.read_hdr()), _bits(want))                          # the second model is in the picture


def test_slot_8_is_refused_and_slot_7_is_not(mesh_dir):
    rp = B.RayPass(B.ladder_from_base((24, 14), 3, 2), device=0)
    m = _model(mesh_dir, 3, A, 1)
    rp.upload_model(m, 7)
    rp.set_model_transform(A, 1, index=7)
    for call in (lambda: rp.upload_model(m, 8), lambda: rp.set_model_transform(A, 1, index=8),
                 lambda: rp.upload_model_uniform(b"\0" * B.layouts.MODEL_UNIFORM_BYTES, 8)):
        with pytest.raises(B.BhrayError):
            call()
    r = B.Renderer(B.ladder_from_base((24, 14), 3, 2), device=0)
    for k in range(B.layouts.MAX_MODELS):
        assert r.add_model(m) == k
    with pytest.raises(ValueError):
        r.add_model(m)
    rp.close()
