"""CPU: the tree of DESIGN.md §12 (the one bhray_upload_model_build builds on the GPU), restated in NumPy (tests/lbvh_ref.py).

The restated tree is a valid BVH of the project's format on every mesh the device build is later held to, and the C oracle, given that
tree in place of the reference's, classifies every pixel as it does with the reference tree.  tests/test_gpu_device_bvh.py then holds
the device build to this restatement byte for byte."""
import numpy as np
import pytest

import bhusie_amd as B
from oracle import oracle as O
from tests import common as T
from tests import lbvh_ref as R
from tests.test_host import _check_bvh_invariants


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("lbvh_meshes")


@pytest.mark.parametrize("name", R.CASES)
def test_restated_tree_is_a_valid_bvh(mesh_dir, name):
    a = R.case_arrays(name, mesh_dir)
    tree = R.build(a["points"], a["triangles"])
    nodes = tree["nodes"]
    if len(a["triangles"]) <= 30000:
        _check_bvh_invariants(R.with_tree(a, tree))
    else:                                                          # the bench mesh: the same invariants, vectorised
        assert sorted(tree["bvh_lookup"].tolist()) == list(range(len(a["triangles"])))
        leaf = nodes["obj_count"] > 0
        starts = np.sort(nodes["left_child"][leaf])
        sizes = nodes["obj_count"][leaf][np.argsort(nodes["left_child"][leaf])]
        assert starts[0] == 0 and np.array_equal(starts[1:], (starts + sizes)[:-1]) and starts[-1] + sizes[-1] == len(a["triangles"])
        P = a["points"][a["triangles"][tree["bvh_lookup"], :3], :3]                       # (T, 3, 3) in sorted order
        order = np.argsort(nodes["left_child"][leaf])
        assert np.array_equal(np.minimum.reduceat(P.min(axis=1), starts, axis=0), nodes["min_corner"][leaf][order])
        assert np.array_equal(np.maximum.reduceat(P.max(axis=1), starts, axis=0), nodes["max_corner"][leaf][order])
    assert int(nodes["obj_count"].max()) <= R.LEAF
    inner = np.nonzero(nodes["obj_count"] == 0)[0] if len(nodes) > 1 else np.zeros(0, dtype=np.int64)
    l = nodes["left_child"][inner]
    assert np.array_equal(nodes["min_corner"][inner], np.minimum(nodes["min_corner"][l], nodes["min_corner"][l + 1]))
    assert np.array_equal(nodes["max_corner"][inner], np.maximum(nodes["max_corner"][l], nodes["max_corner"][l + 1]))
    assert np.array_equal(R.renumber_bfs(nodes), nodes)            # build() numbers breadth-first; every node is reachable once
    assert R.tree_stats(nodes) == (tree["leaves"], tree["max_leaf"], tree["max_depth"])
    assert tree["max_depth"] <= 50
    assert len(nodes) == 2 * tree["leaves"] - 1
    if len(a["triangles"]) <= R.LEAF:
        assert len(nodes) == 1 and nodes[0]["obj_count"] == len(a["triangles"])


def test_special_meshes_split_as_the_rules_say(mesh_dir):
    same = R.build(**{k: R.case_arrays("identical_4097", mesh_dir)[k] for k in ("points", "triangles")})
    assert (len(same["nodes"]), same["max_depth"]) == (2049, 12)   # equal Morton codes: the index bits split
    assert np.array_equal(same["bvh_lookup"], np.arange(4097))
    flat = R.build(**{k: R.case_arrays("lattice", mesh_dir)[k] for k in ("points", "triangles")})
    assert len(flat["nodes"]) == 1023 and np.all(flat["nodes"]["obj_count"][flat["nodes"]["obj_count"] > 0] == 4)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("name", R.CASES[:3])
def test_oracle_classifies_every_pixel_as_with_the_reference_tree(mesh_dir, tmp_path, name, method):
    a = R.case_arrays(name, mesh_dir)
    model = B.load_model(str(mesh_dir / (name + ".obj")))          # the reference tree (and the default model position)
    ref_arrays = model.arrays()
    assert np.array_equal(ref_arrays["points"], a["points"]) and np.array_equal(ref_arrays["triangles"], a["triangles"])
    tree = R.build(a["points"], a["triangles"])
    d = np.array([0.0, -0.04, 1.0]); d /= np.linalg.norm(d)
    cam = B.Camera(position=(-10.0, 1.0, 12.0), forward=tuple(d), fov=1.0)
    u = T.uniforms(camera=cam, integration_method=method, model_count=1)
    cfg = B.ladder_from_base((40, 24), 3, 2)
    tex = T.textures()
    want = O.render_ladder(T.oracle_scene(*u, tex, [ref_arrays]), cfg.sizes())[-1]
    got = O.render_ladder(T.oracle_scene(*u, tex, [R.with_tree(ref_arrays, tree)]), cfg.sizes())[-1]
    bare = O.render_ladder(T.oracle_scene(*T.uniforms(camera=cam, integration_method=method, model_count=0), tex), cfg.sizes())[-1]
    mesh_pixels = int((bare.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    same = float((got.view(np.uint32) == want.view(np.uint32)).all(axis=-1).mean())
    print(f"{name} method {method}: {mesh_pixels} of {want.shape[0] * want.shape[1]} pixels show the mesh; bit-identical to the reference-tree frame: {100.0 * same:.3f} %")
    assert mesh_pixels > 300
    assert np.array_equal(got[..., 3], want[..., 3]), "pixel class differs from the reference-tree frame"
