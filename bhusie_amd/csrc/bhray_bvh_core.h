// bhray_bvh_core.h — the per-element steps of the device LBVH builder, one function per kernel body.
//
// Every function handles ONE element (a triangle, a radix-tree node, a BVH node) and is plain C++: bhray_bvh.hip wraps each in a
// gfx950 kernel, and a host program can run the same text element by element to check the rules without a GPU.  All float work is
// single binary32 operations in the order §12 states (-ffp-contract=off); min / max go through bvh_ord so that they are exact and
// total (-0 below +0) and can be combined in any order.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define BVH_HD __host__ __device__ inline
#else
#define BVH_HD inline
#endif

#define BHRAY_LBVH_LEAF 4            // a range of at most this many sorted keys is a leaf (§12 rule 5)
#define BHRAY_LBVH_MAX_PASSES 50     // tree levels a build can produce: 30 Morton bits + 19 index bits + the leaf (§12 rule 7)

namespace bhray {

struct alignas(16) BvhF4 { float x, y, z, w; };     // layout of float4 (points, normals, node halves, leaf records)
struct BvhRange { int first, last, split, big; };   // one inner node of the binary radix tree: its key range, where it splits, size > BHRAY_LBVH_LEAF

// order-preserving map binary32 -> int32 (its own inverse): a < b <=> ord(a) < ord(b), and -0 < +0
BVH_HD int bvh_ord(float f) { int b; memcpy(&b, &f, 4); return b >= 0 ? b : b ^ 0x7fffffff; }
BVH_HD float bvh_unord(int k) { int b = k >= 0 ? k : k ^ 0x7fffffff; float f; memcpy(&f, &b, 4); return f; }
BVH_HD int bvh_imin(int a, int b) { return a < b ? a : b; }
BVH_HD int bvh_imax(int a, int b) { return a > b ? a : b; }

// rule 1: the triangle's box in ord space, lo[3] / hi[3]
BVH_HD void bvh_triangle_box(const BvhF4* points, const int32_t* tri6, int lo[3], int hi[3]) {
    const BvhF4 a = points[tri6[0]], b = points[tri6[1]], c = points[tri6[2]];
    const int ax = bvh_ord(a.x), ay = bvh_ord(a.y), az = bvh_ord(a.z);
    const int bx = bvh_ord(b.x), by = bvh_ord(b.y), bz = bvh_ord(b.z);
    const int cx = bvh_ord(c.x), cy = bvh_ord(c.y), cz = bvh_ord(c.z);
    lo[0] = bvh_imin(ax, bvh_imin(bx, cx)); lo[1] = bvh_imin(ay, bvh_imin(by, cy)); lo[2] = bvh_imin(az, bvh_imin(bz, cz));
    hi[0] = bvh_imax(ax, bvh_imax(bx, cx)); hi[1] = bvh_imax(ay, bvh_imax(by, cy)); hi[2] = bvh_imax(az, bvh_imax(bz, cz));
}
// rule 1: sort point c = tmin + tmax
BVH_HD void bvh_sort_point(const BvhF4* points, const int32_t* tri6, float c[3]) {
    int lo[3], hi[3];
    bvh_triangle_box(points, tri6, lo, hi);
    for (int a = 0; a < 3; a++) c[a] = bvh_unord(lo[a]) + bvh_unord(hi[a]);
}
BVH_HD bool bvh_triangle_valid(const int32_t* t, int points, int normals) {
    return t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[0] < points && t[1] < points && t[2] < points &&
           t[3] >= 0 && t[4] >= 0 && t[5] >= 0 && t[3] < normals && t[4] < normals && t[5] < normals;
}
BVH_HD uint32_t bvh_spread3(uint32_t v) {           // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// rules 2 and 3: the 30-bit Morton code of a sort point; bounds = ord(lo[3]), ord(hi[3])
BVH_HD uint32_t bvh_morton(const float c[3], const int bounds[6]) {
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float lo = bvh_unord(bounds[a]), hi = bvh_unord(bounds[3 + a]);
        const float ext = hi - lo;
        const float scale = hi == lo ? 0.0f : 1024.0f / ext;
        const float d = c[a] - lo;
        const float s = d * scale;
        uint32_t v = s >= 1023.0f ? 1023u : (s > 0.0f ? (uint32_t)s : 0u);      // min(1023, (uint)s); s is never negative for finite input
        q[a] = v;
    }
    return (bvh_spread3(q[0]) << 2) | (bvh_spread3(q[1]) << 1) | bvh_spread3(q[2]);
}

// rule 4: inner node i of the binary radix tree over the T sorted keys (morton[k] << 32 | tri[k]), T >= 2 (Karras 2012, fig. 4)
BVH_HD int bvh_clz64(uint64_t x) { return __builtin_clzll(x); }
BVH_HD int bvh_delta(const uint32_t* morton, const int32_t* tri, int T, int i, int j) {
    if (j < 0 || j >= T) return -1;
    const uint64_t a = ((uint64_t)morton[i] << 32) | (uint32_t)tri[i], b = ((uint64_t)morton[j] << 32) | (uint32_t)tri[j];
    return bvh_clz64(a ^ b);                          // the keys are distinct: a ^ b != 0
}
BVH_HD BvhRange bvh_radix_node(const uint32_t* morton, const int32_t* tri, int T, int i) {
    const int d = bvh_delta(morton, tri, T, i, i + 1) > bvh_delta(morton, tri, T, i, i - 1) ? 1 : -1;
    const int dmin = bvh_delta(morton, tri, T, i, i - d);
    int lmax = 2;
    while (bvh_delta(morton, tri, T, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (bvh_delta(morton, tri, T, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = bvh_delta(morton, tri, T, i, j);
    int s = 0;
    for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (bvh_delta(morton, tri, T, i, i + (s + t) * d) > dnode) s += t;
        if (t == 1) break;
    }
    BvhRange r;
    r.split = i + s * d + (d < 0 ? -1 : 0);
    r.first = d > 0 ? i : j; r.last = d > 0 ? j : i;
    r.big = (r.last - r.first + 1) > BHRAY_LBVH_LEAF ? 1 : 0;
    return r;
}

// rule 6: a leaf over the sorted positions [lo, hi]: exact box of its triangles' points
BVH_HD void bvh_write_leaf(BvhF4* nodes, int n, const BvhF4* points, const int32_t* triangles, const int32_t* lookup, int lo, int hi) {
    int blo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, bhi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    for (int k = lo; k <= hi; k++) {
        int tlo[3], thi[3];
        bvh_triangle_box(points, triangles + 6 * (size_t)lookup[k], tlo, thi);
        for (int a = 0; a < 3; a++) { blo[a] = bvh_imin(blo[a], tlo[a]); bhi[a] = bvh_imax(bhi[a], thi[a]); }
    }
    int32_t lc = lo, oc = hi - lo + 1;
    BvhF4 h0 = {bvh_unord(blo[0]), bvh_unord(blo[1]), bvh_unord(blo[2]), 0.0f}, h1 = {bvh_unord(bhi[0]), bvh_unord(bhi[1]), bvh_unord(bhi[2]), 0.0f};
    memcpy(&h0.w, &lc, 4); memcpy(&h1.w, &oc, 4);
    nodes[2 * (size_t)n] = h0; nodes[2 * (size_t)n + 1] = h1;
}
BVH_HD void bvh_write_inner_header(BvhF4* nodes, int n, int32_t left_child) {
    BvhF4 h0 = {0.0f, 0.0f, 0.0f, 0.0f}, h1 = {0.0f, 0.0f, 0.0f, 0.0f};           // obj_count 0; the box is fitted later
    memcpy(&h0.w, &left_child, 4);
    nodes[2 * (size_t)n] = h0; nodes[2 * (size_t)n + 1] = h1;
}
// Rules 5 and 8: radix node i with more than BHRAY_LBVH_LEAF keys is an inner BVH node; its two children are BVH nodes 1 + 2 rank[i] and
// 2 + 2 rank[i] (rank = how many such radix nodes have a smaller index).  Writes both children: a child of at most BHRAY_LBVH_LEAF keys as
// a finished leaf (level 1), a larger one as an inner header (level 0).  Returns through leaf_sizes[2] the sizes of the leaves written (0: none).
BVH_HD void bvh_emit_children(const BvhRange* ranges, const int32_t* rank, int i, BvhF4* nodes, int32_t* level, const BvhF4* points,
                              const int32_t* triangles, const int32_t* lookup, int leaf_sizes[2]) {
    const BvhRange r = ranges[i];
    const int base = 1 + 2 * rank[i];
    if (i == 0) { bvh_write_inner_header(nodes, 0, 1); level[0] = 0; }
    for (int c = 0; c < 2; c++) {
        const int lo = c == 0 ? r.first : r.split + 1, hi = c == 0 ? r.split : r.last;
        const int j = c == 0 ? r.split : r.split + 1;             // the child's radix node when it holds more than one key
        const int n = base + c;
        if (hi - lo + 1 <= BHRAY_LBVH_LEAF) {
            bvh_write_leaf(nodes, n, points, triangles, lookup, lo, hi);
            level[n] = 1; leaf_sizes[c] = hi - lo + 1;
        } else {
            bvh_write_inner_header(nodes, n, 1 + 2 * rank[j]);
            level[n] = 0; leaf_sizes[c] = 0;
        }
    }
}
// Rule 6, one pass: BVH node n gets its box in pass p when both children got theirs in an EARLIER pass (level 1 .. p-1).  A child fitted in
// this same pass reads as 0 or p: not yet.  level[n] becomes p = 1 + the larger child level: the node's height in nodes.
BVH_HD bool bvh_fit_node(BvhF4* nodes, int32_t* level, int n, int p) {
    if (level[n] != 0) return false;
    BvhF4 h0 = nodes[2 * (size_t)n], h1 = nodes[2 * (size_t)n + 1];
    int32_t lc; memcpy(&lc, &h0.w, 4);
    const int la = level[lc], lb = level[lc + 1];
    if (la < 1 || la >= p || lb < 1 || lb >= p) return false;
    const BvhF4 a0 = nodes[2 * (size_t)lc], a1 = nodes[2 * (size_t)lc + 1], b0 = nodes[2 * (size_t)lc + 2], b1 = nodes[2 * (size_t)lc + 3];
    h0.x = bvh_unord(bvh_imin(bvh_ord(a0.x), bvh_ord(b0.x))); h0.y = bvh_unord(bvh_imin(bvh_ord(a0.y), bvh_ord(b0.y))); h0.z = bvh_unord(bvh_imin(bvh_ord(a0.z), bvh_ord(b0.z)));
    h1.x = bvh_unord(bvh_imax(bvh_ord(a1.x), bvh_ord(b1.x))); h1.y = bvh_unord(bvh_imax(bvh_ord(a1.y), bvh_ord(b1.y))); h1.z = bvh_unord(bvh_imax(bvh_ord(a1.z), bvh_ord(b1.z)));
    nodes[2 * (size_t)n] = h0; nodes[2 * (size_t)n + 1] = h1;
    level[n] = p;
    return true;
}
// the 96-byte leaf record of sorted position k: the three points, then the three normals, of triangle lookup[k] (copies)
BVH_HD void bvh_gather_leaf(BvhF4* leaf, int k, const BvhF4* points, const BvhF4* normals, const int32_t* triangles, const int32_t* lookup) {
    const int32_t* t = triangles + 6 * (size_t)lookup[k];
    BvhF4* o = leaf + 6 * (size_t)k;
    o[0] = points[t[0]]; o[1] = points[t[1]]; o[2] = points[t[2]];
    o[3] = normals[t[3]]; o[4] = normals[t[4]]; o[5] = normals[t[5]];
}

}  // namespace bhray
