"""CPU: the NumPy reference of the lensed-mesh mode (tests/lensed_ref.py) against the restatement it was copied from.

Where the one changed literal cannot matter - no model, or a model that no segment inside the relativity sphere can reach - it must be
oracle.np_ray's frame bit for bit; where a model stands inside the sphere it must draw it."""
import numpy as np

import bhusie_amd as B
from bhusie_amd import assets
from oracle import np_ray as N
from tests import common as T
from tests import lensed_ref as LR

SIZES = [(32, 18)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _mesh(tmp_path, radius, pos):
    p = tmp_path / f"ico1_{radius}.obj"
    p.write_text(assets.icosphere_mesh_obj(1, radius=float(radius)))          # 80 triangles
    m = B.load_model(str(p))
    m.set_transform(pos, 1)
    return m.arrays()


def test_no_model_is_the_plain_frame_bit_for_bit():
    tex = T.textures()
    for method in (1, 0):
        S = N.Scene(*T.uniforms(integration_method=method, model_count=0), *tex)
        a, b = {}, {}
        want = N.render_ladder(S, [(16, 9), (46, 25)], a)
        got = LR.render_ladder_lensed(S, [(16, 9), (46, 25)], b)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g), _bits(w))
        assert b.pop("segment_hits") == 0 and a == b
    assert N.trace_rays is not LR.trace_rays_lensed                          # the swap is undone


def test_a_mesh_beyond_the_sphere_is_the_plain_frame_bit_for_bit(tmp_path):
    """R = 20, mesh radius 8 (bump 0.15: within 9.2 of its centre) at distance 36: wholly beyond R + 5, and a step's segment starts inside R
    and is shorter than 5 - the lensed test finds nothing, the flat phase finds what it always found."""
    tex = T.textures()
    arrays = _mesh(tmp_path, 8, (-10.0, 0.0, 34.6))
    far = np.linalg.norm(arrays["points"][:, :3] + np.array(arrays["position"], np.float32), axis=1).min()
    assert far > 25.0
    S = N.Scene(*T.uniforms(integration_method=1, model_count=1), *tex, [arrays])
    a, b = {}, {}
    want = N.render_ladder(S, SIZES, a)[-1]
    got = LR.render_ladder_lensed(S, SIZES, b)[-1]
    assert np.array_equal(_bits(got), _bits(want))
    assert b.pop("segment_hits") == 0 and a == b
    bare = N.render_ladder(N.Scene(*T.uniforms(integration_method=1, model_count=0), *tex), SIZES)[-1]
    assert (_bits(bare) != _bits(want)).any()                                # the mesh is in the picture, through the flat phase


def test_a_mesh_inside_the_sphere_is_drawn(tmp_path):
    """The first scene of tests/test_gpu_lensed.py: a mesh at (3.5, -1.5, -8) in front of the default camera at (0, 0, -19), inside R = 20, where
    the plain mode never tests it."""
    tex = T.textures()
    S = N.Scene(*T.uniforms(integration_method=1, model_count=1), *tex, [_mesh(tmp_path, 3, (3.5, -1.5, -8.0))])
    st = {}
    plain = N.render_ladder(S, SIZES)[-1]
    lensed = LR.render_ladder_lensed(S, SIZES, st)[-1]
    assert st["segment_hits"] >= 5
    centre = (slice(4, 14), slice(8, 24))                                    # the image-centre region: rows 4-13, columns 8-23 of 18 x 32
    new_colour = (lensed[centre][..., 3] == 1.0) & (plain[centre][..., 3] == 0.0)
    assert int(new_colour.sum()) >= 5
    changed = (_bits(lensed) != _bits(plain)).any(axis=-1)
    assert int(changed.sum()) == st["segment_hits"]                          # one level: a ray ends on its first mesh hit, nothing else moves
