"""NumPy restatement of the device-built tree, written from the text of DESIGN.md §12 (not from the kernels).

build(points, triangles) -> dict(nodes, bvh_lookup, leaves, max_leaf, max_depth): the tree of §12 in breadth-first numbering (root 0,
left before right).  renumber_bfs(nodes) brings any tree of the same format into that numbering, so that two trees can be compared
byte for byte whatever numbering their builder chose (§12 rule 8 leaves it to the builder).

The radix tree over distinct sorted keys is unique (rule 4), so it is written here top-down: a range splits where the highest bit in
which its first and last key differ goes from 0 to 1 (np.searchsorted)."""
from __future__ import annotations

import numpy as np

from bhusie_amd.model import NODE_DTYPE

LEAF = 4                       # rule 5


def _ord(x):
    """order-preserving int32 image of binary32 values: a < b <=> ord(a) < ord(b), -0 below +0 (the total order rules 1, 2, 6 take min / max in)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def _unord(k):
    k = np.ascontiguousarray(k, dtype=np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)


def _spread3(v):
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for bit in range(10):
        out |= ((v >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit)
    return out


def sort_keys(points, triangles):
    """rules 1-3: (64-bit keys per triangle, per-triangle ord boxes lo / hi)"""
    P = _ord(np.asarray(points, dtype=np.float32)[:, :3])
    tri = np.asarray(triangles, dtype=np.int64)[:, :3]
    corners = P[tri]                                               # (T, 3 corners, 3 axes), ord space
    tlo, thi = corners.min(axis=1), corners.max(axis=1)
    c = (_unord(tlo) + _unord(thi)).astype(np.float32)             # rule 1: one f32 add per axis
    lo, hi = _unord(_ord(c).min(axis=0)), _unord(_ord(c).max(axis=0))
    q = np.zeros(c.shape, dtype=np.uint64)
    for a in range(3):
        ext = np.float32(hi[a] - lo[a])
        scale = np.float32(0.0) if hi[a] == lo[a] else np.float32(np.float32(1024.0) / ext)
        s = ((c[:, a] - lo[a]).astype(np.float32) * scale).astype(np.float32)
        q[:, a] = np.minimum(1023, s.astype(np.int64)).astype(np.uint64)
    morton = (_spread3(q[:, 0]) << np.uint64(2)) | (_spread3(q[:, 1]) << np.uint64(1)) | _spread3(q[:, 2])
    keys = (morton << np.uint64(32)) | np.arange(len(tri), dtype=np.uint64)
    return keys, tlo, thi


def build(points, triangles):
    T = len(triangles)
    assert T >= 1
    keys, tlo, thi = sort_keys(points, triangles)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    slo, shi = tlo[order], thi[order]
    # rules 4, 5, 8 (breadth-first): queue of ranges
    first, last, left = [0], [T - 1], []
    depth = [1]
    q = 0
    while q < len(first):
        a, b = first[q], last[q]
        if b - a + 1 <= LEAF:
            left.append(-1)
        else:
            h = int(sk[a] ^ sk[b]).bit_length() - 1                # the highest differing bit
            v = ((int(sk[a]) >> h) | 1) << h                       # the first key of the range with that bit set
            pos = a + int(np.searchsorted(sk[a:b + 1], np.uint64(v), side="left"))
            left.append(len(first))
            first += [a, pos]; last += [pos - 1, b]; depth += [depth[q] + 1] * 2
        q += 1
    n = len(first)
    first, last, left = np.array(first), np.array(last), np.array(left)
    is_leaf = left < 0
    lo = np.zeros((n, 3), dtype=np.int32); hi = np.zeros((n, 3), dtype=np.int32)
    # rule 6: leaves from their triangles (the leaves tile the sorted order) ...
    li = np.nonzero(is_leaf)[0]
    li = li[np.argsort(first[li])]
    lo[li] = np.minimum.reduceat(slo, first[li], axis=0)
    hi[li] = np.maximum.reduceat(shi, first[li], axis=0)
    # ... inner nodes from their children (children have larger breadth-first numbers)
    for i in range(n - 1, -1, -1):
        if not is_leaf[i]:
            l = left[i]
            lo[i] = np.minimum(lo[l], lo[l + 1]); hi[i] = np.maximum(hi[l], hi[l + 1])
    nodes = np.zeros(n, dtype=NODE_DTYPE)
    nodes["min_corner"] = _unord(lo.reshape(-1)).reshape(n, 3)
    nodes["max_corner"] = _unord(hi.reshape(-1)).reshape(n, 3)
    nodes["left_child"] = np.where(is_leaf, first, left)
    nodes["obj_count"] = np.where(is_leaf, last - first + 1, 0)
    sizes = (last - first + 1)[is_leaf]
    return dict(nodes=nodes, bvh_lookup=order.astype(np.int32), leaves=int(is_leaf.sum()), max_leaf=int(sizes.max()), max_depth=int(max(depth)))


def renumber_bfs(nodes):
    """the same tree numbered breadth-first from the root, left before right (leaf ranges untouched)"""
    nodes = np.asarray(nodes)
    order, q = [0], 0
    new_left = []
    while q < len(order):
        nd = nodes[order[q]]
        if nd["obj_count"] == 0:
            new_left.append(len(order))
            order += [int(nd["left_child"]), int(nd["left_child"]) + 1]
        else:
            new_left.append(int(nd["left_child"]))
        q += 1
    assert len(order) == len(nodes) and len(set(order)) == len(nodes), "unreachable or shared nodes"
    out = nodes[np.array(order)].copy()
    out["left_child"] = np.array(new_left, dtype=np.int32)
    return out


def tree_stats(nodes):
    """(leaves, max_leaf, max_depth) of any tree; max_depth counts the nodes on the longest path root -> leaf"""
    nodes = np.asarray(nodes)
    depth = np.zeros(len(nodes), dtype=np.int64)
    depth[0] = 1
    stack = [0]
    while stack:
        i = stack.pop()
        if nodes[i]["obj_count"] == 0:
            l = int(nodes[i]["left_child"])
            depth[l] = depth[l + 1] = depth[i] + 1
            stack += [l, l + 1]
    leaf = nodes["obj_count"] > 0
    return int(leaf.sum()), int(nodes["obj_count"].max()), int(depth.max())


# ---- the meshes the tree is checked on (tests/test_device_bvh_ref.py on the CPU, tests/test_gpu_device_bvh.py on the device)
CASES = ("sphere_24_32", "sphere_40_48", "ico4", "ico5", "bench", "one", "four", "five", "identical_4097", "lattice", "doubled")


def _raw(points, triangles, normals=None):
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.shape[1] == 3:
        points = np.concatenate([points, np.zeros((len(points), 1), np.float32)], axis=1)
    if normals is None:
        normals = np.array([[0.0, 0.0, 1.0, 0.0]], dtype=np.float32)
    tri = np.zeros((len(triangles), 6), dtype=np.int32)
    tri[:, :np.shape(triangles)[1]] = triangles
    return dict(position=np.array((-10.0, 0.0, 30.0), np.float32), visible=1, points=points, normals=np.ascontiguousarray(normals, dtype=np.float32), triangles=tri)


def case_arrays(name, tmp_dir):
    """dict(position, visible, points, normals, triangles) of one named mesh; OBJ meshes go through the product's loader"""
    import os

    import bhusie_amd as B
    from bhusie_amd import assets
    obj = {"sphere_24_32": lambda: assets.sphere_mesh_obj(24, 32, radius=8.0, bump=0.2, seed=5),
           "sphere_40_48": lambda: assets.sphere_mesh_obj(40, 48, radius=7.0, bump=0.2, seed=9),
           "ico4": lambda: assets.icosphere_mesh_obj(4, radius=8.0, bump=0.15, seed=3),
           "ico5": lambda: assets.icosphere_mesh_obj(5, radius=8.0, bump=0.15, seed=3),
           "bench": lambda: assets.icosphere_mesh_obj(7, radius=8.0, bump=0.15, seed=3)}
    if name in obj:
        p = os.path.join(str(tmp_dir), name + ".obj")
        if not os.path.exists(p):
            with open(p, "w") as f:
                f.write(obj[name]())
        a = B.load_model(p).arrays()
        return {k: a[k] for k in ("position", "visible", "points", "normals", "triangles")}
    tri_pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, -0.5]], np.float32)
    if name in ("one", "four", "five"):
        n = {"one": 1, "four": 4, "five": 5}[name]
        pts = np.concatenate([tri_pts + np.float32(1.5 * k) * np.array([1.0, -0.5, 0.25], np.float32) for k in range(n)])
        return _raw(pts, np.arange(3 * n).reshape(n, 3))
    if name == "identical_4097":
        return _raw(tri_pts, np.tile(np.array([[0, 1, 2]]), (4097, 1)))
    if name == "lattice":                                          # planar: one axis with hi == lo
        g = 33
        ys, xs = np.mgrid[0:g, 0:g]
        pts = np.stack([xs.ravel() * 0.5, np.full(g * g, 2.0), ys.ravel() * 0.25], axis=1)
        a = (ys[:-1, :-1] * g + xs[:-1, :-1]).ravel()
        tri = np.concatenate([np.stack([a, a + 1, a + g + 1], 1), np.stack([a, a + g + 1, a + g], 1)])
        return _raw(pts, tri)
    if name == "doubled":                                          # every triangle present twice
        a = case_arrays("sphere_24_32", tmp_dir)
        a["triangles"] = np.concatenate([a["triangles"], a["triangles"]])
        return a
    raise KeyError(name)


def with_tree(arrays, tree):
    """the model dict the oracle takes: `arrays` with the tree's nodes and bvh_lookup"""
    out = dict(arrays)
    out["nodes"], out["bvh_lookup"] = tree["nodes"], tree["bvh_lookup"]
    return out
