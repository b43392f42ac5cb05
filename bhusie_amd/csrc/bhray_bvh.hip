// bhray_bvh.hip — the mesh BVH built on the GPU (gfx950, wave64): the LBVH of DESIGN.md §12.
//
// One build = index validation (its own launch, read back before anything reads through an index), then on one stream:
//   bounds of the sort points -> Morton codes -> stable radix sort by the 30 Morton bits (triangle index as the value: the order of the
//   64-bit keys morton << 32 | index) -> the binary radix tree, one thread per inner node -> a scan numbers the nodes that keep more than
//   BHRAY_LBVH_LEAF keys -> every such node writes its two children (leaves finished, inner nodes as headers) -> the boxes of the inner
//   nodes, bottom-up in PASSES: one launch per tree height, a node is fitted by the launch after the one that fitted its second child.
//   Nothing is handed from one workgroup to another inside a launch (kernel boundaries order every read after the write it needs), no
//   wave waits for another, min / max are exact: the bytes do not depend on scheduling, device or run.
//   -> the 96-byte leaf records -> 64 bytes of result (counts, depth, the root-children union for ModelDev::root_cull).
// The per-element steps are bhray_bvh_core.h (plain C++ that a host program can run as well).
// launch_bvh_pose writes a slot's points and normals from its rest arrays and a 3x4 affine pose; the build above then runs on the result.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bhray_bvh_core.h"
#include "bhray_internal.h"

namespace bhray {

struct BvhBuild {
    int T = 0;
    uint32_t* morton_in = nullptr; uint32_t* morton = nullptr;     // per triangle / per sorted position
    int32_t* index_in = nullptr;                                   // 0 .. T-1
    BvhRange* ranges = nullptr;                                    // [T-1] radix-tree nodes
    int32_t* big = nullptr; int32_t* rank = nullptr;               // [T-1] keeps more than BHRAY_LBVH_LEAF keys / exclusive scan of that
    int32_t* level = nullptr;                                      // [2T-1] per BVH node: 0 = box not fitted yet, else the pass that fitted it (leaf = 1)
    int* state = nullptr;                                          // [0..5] ord bounds of the sort points, [6] leaves, [7] largest leaf, [8] validation error
    void* tmp = nullptr; size_t tmp_bytes = 0;                     // rocprim scratch (the larger of sort and scan)
};
enum { ST_LEAVES = 6, ST_MAX_LEAF = 7, ST_ERROR = 8, ST_WORDS = 16 };

namespace {

constexpr int BLOCK = 256;
inline int blocks_for(int n) { return (n + BLOCK - 1) / BLOCK; }
inline const BvhF4* F4(const float4* p) { return reinterpret_cast<const BvhF4*>(p); }
inline BvhF4* F4(float4* p) { return reinterpret_cast<BvhF4*>(p); }

__device__ inline int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ inline int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }

__global__ __launch_bounds__(BLOCK) void bvh_validate_kernel(const int32_t* triangles, int T, int P, int N, int* state) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const bool bad = t < T && !bvh_triangle_valid(triangles + 6 * (size_t)t, P, N);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&state[ST_ERROR], 1);
}
__global__ void bvh_reset_kernel(int* state) {
    const int i = threadIdx.x;
    if (i < 3) state[i] = 0x7fffffff;
    else if (i < 6) state[i] = (int)0x80000000;
    else if (i < ST_WORDS) state[i] = 0;
}
__global__ __launch_bounds__(BLOCK) void bvh_bounds_kernel(const BvhF4* points, const int32_t* triangles, int T, int* state) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    if (t < T) {
        float c[3];
        bvh_sort_point(points, triangles + 6 * (size_t)t, c);
        for (int a = 0; a < 3; a++) lo[a] = hi[a] = bvh_ord(c[a]);
    }
    for (int a = 0; a < 3; a++) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if ((threadIdx.x & 63) == 0) {                                  // integer min / max: exact and independent of the order of arrival
        for (int a = 0; a < 3; a++) { atomicMin(&state[a], lo[a]); atomicMax(&state[3 + a], hi[a]); }
    }
}
__global__ __launch_bounds__(BLOCK) void bvh_keys_kernel(const BvhF4* points, const int32_t* triangles, int T, const int* state,
                                                         uint32_t* morton_in, int32_t* index_in) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    int bounds[6];
    for (int a = 0; a < 6; a++) bounds[a] = state[a];
    float c[3];
    bvh_sort_point(points, triangles + 6 * (size_t)t, c);
    morton_in[t] = bvh_morton(c, bounds);
    index_in[t] = t;
}
__global__ __launch_bounds__(BLOCK) void bvh_radix_kernel(const uint32_t* morton, const int32_t* lookup, int T, BvhRange* ranges, int32_t* big) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= T - 1) return;
    const BvhRange r = bvh_radix_node(morton, lookup, T, i);
    ranges[i] = r;
    big[i] = r.big;
}
__global__ __launch_bounds__(BLOCK) void bvh_emit_kernel(const BvhRange* ranges, const int32_t* big, const int32_t* rank, int T, BvhF4* nodes, int32_t* level,
                                                         const BvhF4* points, const int32_t* triangles, const int32_t* lookup, int* state) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    int leaves = 0, largest = 0;
    if (i < T - 1 && big[i] != 0) {
        int sz[2];
        bvh_emit_children(ranges, rank, i, nodes, level, points, triangles, lookup, sz);
        leaves = (sz[0] > 0) + (sz[1] > 0);
        largest = max(sz[0], sz[1]);
    }
    largest = wave_max(largest);
    for (int o = 32; o > 0; o >>= 1) leaves += __shfl_xor(leaves, o);
    if ((threadIdx.x & 63) == 0 && leaves > 0) { atomicAdd(&state[ST_LEAVES], leaves); atomicMax(&state[ST_MAX_LEAF], largest); }
}
// T <= BHRAY_LBVH_LEAF: the root is the only node and a leaf
__global__ void bvh_single_leaf_kernel(int T, BvhF4* nodes, int32_t* level, const BvhF4* points, const int32_t* triangles, const int32_t* lookup, int* state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bvh_write_leaf(nodes, 0, points, triangles, lookup, 0, T - 1);
    level[0] = 1; state[ST_LEAVES] = 1; state[ST_MAX_LEAF] = T;
}
__global__ __launch_bounds__(BLOCK) void bvh_fit_kernel(BvhF4* nodes, int32_t* level, const int32_t* big, const int32_t* rank, int T, int pass) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    const int count = 1 + 2 * (rank[T - 2] + big[T - 2]);
    if (n >= count) return;
    bvh_fit_node(nodes, level, n, pass);
}
__global__ __launch_bounds__(BLOCK) void bvh_leaf_records_kernel(BvhF4* leaf, int T, const BvhF4* points, const BvhF4* normals, const int32_t* triangles, const int32_t* lookup) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k < T) bvh_gather_leaf(leaf, k, points, normals, triangles, lookup);
}
__global__ void bvh_result_kernel(const BvhF4* nodes, const int32_t* level, const int32_t* big, const int32_t* rank, int T, const int* state, BvhResult* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    BvhResult r;
    memset(&r, 0, sizeof r);
    r.nodes = T > BHRAY_LBVH_LEAF ? 1u + 2u * (uint32_t)(rank[T - 2] + big[T - 2]) : 1u;
    r.leaves = (uint32_t)state[ST_LEAVES]; r.max_leaf = (uint32_t)state[ST_MAX_LEAF];
    r.max_depth = (uint32_t)level[0];                              // 0: the passes did not reach the root (cannot happen within the capacities, §12 rule 7)
    if (r.nodes >= 3 && r.max_depth != 0) {
        const BvhF4 a0 = nodes[2], a1 = nodes[3], b0 = nodes[4], b1 = nodes[5];
        const float l1[3] = {a0.x, a0.y, a0.z}, l2[3] = {b0.x, b0.y, b0.z}, h1[3] = {a1.x, a1.y, a1.z}, h2[3] = {b1.x, b1.y, b1.z};
        for (int a = 0; a < 3; a++) { r.root_lo[a] = l1[a] < l2[a] ? l1[a] : l2[a]; r.root_hi[a] = h1[a] > h2[a] ? h1[a] : h2[a]; }   // as dev_upload_model
        bool finite = true;
        for (int a = 0; a < 3; a++) finite = finite && isfinite(r.root_lo[a]) && isfinite(r.root_hi[a]);
        r.root_cull = finite ? 1 : 0;
    }
    *out = r;
}

// The affine pose of a device-built slot: vertex v < P is rest point v, the others are rest normals.  One float4 in, one float4 out per
// thread (lane i at base + 16 i: one 1 KiB access per wave); the 12 pose floats are a kernel argument, wave-uniform, in SGPRs.  One rounded binary32
// operation at a time in the order written (-ffp-contract=off): row r of a point is ((m[4r] x + m[4r+1] y) + m[4r+2] z) + m[4r+3], a normal gets the
// linear part only, w is copied.  The wave that holds the last point and the first normal is the only one whose lanes differ in `point`.
struct BvhPose { float m[12]; };
__global__ __launch_bounds__(BLOCK) void bvh_pose_kernel(const float4* rest_points, const float4* rest_normals, float4* points, float4* normals, int P, int N, BvhPose pose) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= P + N) return;
    const bool point = v < P;
    const float4 in = *(point ? rest_points + v : rest_normals + (v - P));
    float4* const dst = point ? points + v : normals + (v - P);      // one address, so one 16-byte store
    float4 out;
    float r[3];
    for (int a = 0; a < 3; a++) {
        const float lin = ((pose.m[4 * a] * in.x + pose.m[4 * a + 1] * in.y) + pose.m[4 * a + 2] * in.z);
        r[a] = point ? lin + pose.m[4 * a + 3] : lin;
    }
    out.x = r[0]; out.y = r[1]; out.z = r[2]; out.w = in.w;
    *dst = out;
}

}  // namespace

hipError_t launch_bvh_pose(const float4* rest_points, const float4* rest_normals, float4* points, float4* normals, int point_count, int normal_count,
                           const float pose[12], hipStream_t s) {
    if (point_count < 0 || normal_count < 0 || point_count > BHRAY_MAX_MODEL_VERTICES || normal_count > BHRAY_MAX_MODEL_VERTICES) return hipErrorInvalidValue;
    const int n = point_count + normal_count;                      // at most 2^20
    if (n == 0) return hipSuccess;
    BvhPose p;
    memcpy(p.m, pose, sizeof p.m);
    hipLaunchKernelGGL(bvh_pose_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, s, rest_points, rest_normals, points, normals, point_count, normal_count, p);
    return hipGetLastError();
}

void bvh_build_destroy(BvhBuild* b) {
    if (!b) return;
    void* ptrs[] = {b->morton_in, b->morton, b->index_in, b->ranges, b->big, b->rank, b->level, b->state, b->tmp};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete b;
}

hipError_t bvh_build_create(int T, BvhBuild** out) {
    *out = nullptr;
    if (T < 1) return hipErrorInvalidValue;
    BvhBuild* b = new BvhBuild();
    b->T = T;
    const size_t n = (size_t)T, inner = n > 1 ? n - 1 : 1;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    alloc((void**)&b->morton_in, n * 4); alloc((void**)&b->morton, n * 4); alloc((void**)&b->index_in, n * 4);
    alloc((void**)&b->ranges, inner * sizeof(BvhRange)); alloc((void**)&b->big, inner * 4); alloc((void**)&b->rank, inner * 4);
    alloc((void**)&b->level, (2 * n - 1) * 4); alloc((void**)&b->state, ST_WORDS * sizeof(int));
    size_t sort_bytes = 0, scan_bytes = 0;
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, sort_bytes, b->morton_in, b->morton, b->index_in, b->index_in, (unsigned)T, 0u, 30u, (hipStream_t) nullptr);
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, scan_bytes, b->big, b->rank, (int32_t)0, inner, rocprim::plus<int32_t>(), (hipStream_t) nullptr);
    b->tmp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    if (b->tmp_bytes < 16) b->tmp_bytes = 16;
    alloc(&b->tmp, b->tmp_bytes);
    if (e != hipSuccess) { bvh_build_destroy(b); return e; }
    *out = b;
    return hipSuccess;
}

hipError_t launch_bvh_validate(BvhBuild* b, const int32_t* triangles, int P, int N, int* host_error, hipStream_t s) {
    hipLaunchKernelGGL(bvh_reset_kernel, dim3(1), dim3(64), 0, s, b->state);
    hipLaunchKernelGGL(bvh_validate_kernel, dim3(blocks_for(b->T)), dim3(BLOCK), 0, s, triangles, b->T, P, N, b->state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(host_error, b->state + ST_ERROR, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

hipError_t launch_bvh_build(BvhBuild* b, const float4* points, const float4* normals, const int32_t* triangles, float4* nodes, int32_t* lookup, float4* leaf,
                            BvhResult* d_result, hipStream_t s) {
    const int T = b->T;
    const BvhF4* pts = F4(points);
    hipLaunchKernelGGL(bvh_reset_kernel, dim3(1), dim3(64), 0, s, b->state);
    hipLaunchKernelGGL(bvh_bounds_kernel, dim3(blocks_for(T)), dim3(BLOCK), 0, s, pts, triangles, T, b->state);
    hipLaunchKernelGGL(bvh_keys_kernel, dim3(blocks_for(T)), dim3(BLOCK), 0, s, pts, triangles, T, b->state, b->morton_in, b->index_in);
    size_t bytes = b->tmp_bytes;
    // stable, so equal Morton codes keep the ascending triangle index: the order of the 64-bit keys of §12 rule 3
    hipError_t e = rocprim::radix_sort_pairs(b->tmp, bytes, b->morton_in, b->morton, b->index_in, lookup, (unsigned)T, 0u, 30u, s);
    if (e != hipSuccess) return e;
    if (T > BHRAY_LBVH_LEAF) {
        hipLaunchKernelGGL(bvh_radix_kernel, dim3(blocks_for(T - 1)), dim3(BLOCK), 0, s, b->morton, lookup, T, b->ranges, b->big);
        bytes = b->tmp_bytes;
        e = rocprim::exclusive_scan(b->tmp, bytes, b->big, b->rank, (int32_t)0, (size_t)(T - 1), rocprim::plus<int32_t>(), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bvh_emit_kernel, dim3(blocks_for(T - 1)), dim3(BLOCK), 0, s, b->ranges, b->big, b->rank, T, F4(nodes), b->level, pts, triangles, lookup, b->state);
        // a node of height h (leaf = 1) is fitted by pass h; no tree of these keys is higher than BHRAY_LBVH_MAX_PASSES
        for (int pass = 2; pass <= BHRAY_LBVH_MAX_PASSES; pass++)
            hipLaunchKernelGGL(bvh_fit_kernel, dim3(blocks_for(2 * T - 1)), dim3(BLOCK), 0, s, F4(nodes), b->level, b->big, b->rank, T, pass);
    } else {
        hipLaunchKernelGGL(bvh_single_leaf_kernel, dim3(1), dim3(64), 0, s, T, F4(nodes), b->level, pts, triangles, lookup, b->state);
    }
    hipLaunchKernelGGL(bvh_leaf_records_kernel, dim3(blocks_for(T)), dim3(BLOCK), 0, s, F4(leaf), T, pts, F4(normals), triangles, lookup);
    hipLaunchKernelGGL(bvh_result_kernel, dim3(1), dim3(64), 0, s, F4(nodes), b->level, b->big, b->rank, T, b->state, d_result);
    return hipGetLastError();
}

}  // namespace bhray
