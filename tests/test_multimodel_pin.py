"""CPU: several models per scene (BHRAY_MAX_MODELS = 8) against frames made by EXECUTING the reference's own shader text.

tests/golden/multimodel.npz was written by tests/golden/make_golden_multimodel.py: ray.wgsl run by oracle/wgsl_exec.py with 2-4 models
bound (its model loop, ray.wgsl:377-389, over model_count entries), both integrators, two- and three-level ladders, an invisible slot and a
slot never uploaded.  The fixture holds seeds, poses and frames; the meshes are rebuilt here from the seeds.  The C oracle in literal
mode must reproduce every word; where the reference's shader is present a slice of one frame is executed again and must equal the file.
tests/test_gpu_multimodel.py holds the BHRAY_F_LITERAL kernel to the same file.
"""
import os

import numpy as np
import pytest

from bhusie_amd import assets
from oracle import host_oracle as H
from oracle import oracle as O
from oracle import wgsl_exec as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["rk_pair", "euler_four", "rk_holes", "euler_three"]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "multimodel.npz"))


def _placeholder():
    return dict(position=(0.0, 0.0, 0.0), visible=0, points=np.zeros((0, 4), np.float32), normals=np.zeros((0, 4), np.float32),
                triangles=np.zeros((0, 6), np.int32), nodes=np.zeros(32, np.uint8), bvh_lookup=np.zeros(0, np.int32))


def scene_of(g, name, visible_override=None):
    tex = (g["t_temp"], g["t_disk"], g["t_sky"])
    u = tuple(g[f"{name}.{k}"].tobytes() for k in ("camera", "black_hole", "details"))
    sizes = [tuple(int(v) for v in s) for s in g[f"{name}.sizes"]]
    n_lat, n_lon = (int(v) for v in g["mesh_params"])
    radius, bump = (float(v) for v in g["mesh_shape"])
    models = []
    for i, (seed, pos, vis) in enumerate(zip(g[f"{name}.seeds"], g[f"{name}.positions"], g[f"{name}.visible"])):
        if int(seed) < 0:
            models.append(_placeholder())
            continue
        m = H.load_model(assets.sphere_mesh_obj(n_lat, n_lon, radius=radius, bump=bump, seed=int(seed), with_normals=True)).as_oracle_dict()
        m["position"] = tuple(float(v) for v in pos)
        m["visible"] = int(vis) if visible_override is None else visible_override(i, int(vis))
        models.append(m)
    return u, tex, sizes, models


def _literal_ladder(u, tex, sizes, models):
    O.set_eval(O.EVAL_LITERAL)
    try:
        return O.render_ladder(O.OracleScene(*u, *tex, models=models), sizes)
    finally:
        O.set_eval(O.EVAL_CONTRACT)


def test_fixture_covers_the_model_loop(g):
    """Both integrators, 2-4 slots, an invisible slot and one never uploaded, every visible model in the picture, within the size limit."""
    assert os.path.getsize(os.path.join(GOLD, "multimodel.npz")) < 1 << 20
    assert sorted(k[:-6] for k in g.files if k.endswith(".sizes")) == sorted(SCENES)
    methods, counts = set(), set()
    for name in SCENES:
        det = np.frombuffer(g[f"{name}.details"].tobytes(), dtype=np.int32)
        methods.add(int(det[3])); counts.add(int(det[1]))
        assert int(det[1]) == len(g[f"{name}.seeds"]) >= 2
    assert methods == {0, 1} and max(counts) >= 4
    assert (g["rk_holes.seeds"] < 0).any() and ((g["rk_holes.seeds"] >= 0) & (g["rk_holes.visible"] == 0)).any()
    for name in ("euler_three", "rk_pair"):
        u, tex, sizes, models = scene_of(g, name)
        full = g[f"{name}.level{len(sizes) - 1}"]
        for i in range(len(models)):
            _, _, _, less = scene_of(g, name, lambda j, v, i=i: 0 if j == i else v)
            im = _literal_ladder(u, tex, sizes, less)[-1]
            assert int((im != full).any(axis=-1).sum()) > 0, f"{name}: model {i} is not in the picture"


@pytest.mark.parametrize("name", SCENES)
def test_c_oracle_literal_mode_equals_the_executed_shader_word_for_word(g, name):
    u, tex, sizes, models = scene_of(g, name)
    for l, im in enumerate(_literal_ladder(u, tex, sizes, models)):
        want = g[f"{name}.level{l}"]
        bad = (im.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(im) & np.isnan(want))
        assert not bad.any(), f"{name} level {l}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.skipif(not os.path.exists(W.SHADER), reason="the reference's shader is not on this machine")
def test_fixture_is_what_executing_the_shader_text_gives(g):
    ns = W.compile_shader()
    name, level, rows = "euler_three", 2, (30, 32)
    u, tex, sizes, models = scene_of(g, name)
    W.bind_scene(ns, *u, *tex, models)
    got = W.render_level(ns, sizes[level], g[f"{name}.level{level - 1}"], rows)[rows[0]:rows[1]]
    want = g[f"{name}.level{level}"][rows[0]:rows[1]]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
