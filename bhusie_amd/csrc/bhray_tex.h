// bhray_tex.h — the texture sample shared by the trace kernels, the sky pass (bhray_kernels.hip) and the accumulation's resolve, and that resolve (bhray_accum.hip,
// bhray_adapt.hip).
// Device code only; included behind bhray_internal.h (TexDev) and bhray_math.h (mix_).
#pragma once

namespace bhray {

// A texel's byte as unorm: x / 255.0f, or (SEQ) the trace kernels' short exact sequence for it - unorm8_rn, which stays with the other sequences in bhray_kernels.hip
// (a translation unit that only samples with SEQ = false never names it)
__device__ __forceinline__ float unorm8_rn(float x);
template <bool SEQ> __device__ __forceinline__ float unorm8(float x) { if constexpr (SEQ) return unorm8_rn(x); else return x / 255.0f; }

// ------------------------------------------------------------------------------------------
// textures: RGBA8 unorm, bilinear, clamp-to-edge (texture.rs:32,61-69; textureSampleLevel 0)
// (SEQ: the bytes through unorm8_rn - the trace kernels' samples, per build; the sky pass keeps the division)
// ------------------------------------------------------------------------------------------
template <bool SEQ>
__device__ __forceinline__ float4 texel(const TexDev& t, int x, int y) {
    const uchar4 p = *reinterpret_cast<const uchar4*>(t.rgba + 4 * ((size_t)y * (size_t)t.w + (size_t)x));
    return make_float4(unorm8<SEQ>((float)p.x), unorm8<SEQ>((float)p.y), unorm8<SEQ>((float)p.z), unorm8<SEQ>((float)p.w));
}
__device__ __forceinline__ float unit_coord(float u, int n, int& i0, int& i1) {
    float x = u * (float)n - 0.5f;
    if (!(x >= -1.0f)) x = -1.0f;
    if (x > (float)n) x = (float)n;
    float fl = floorf(x);
    int a = (int)fl, b = a + 1;
    a = a < 0 ? 0 : a; a = a > n - 1 ? n - 1 : a;
    b = b < 0 ? 0 : b; b = b > n - 1 ? n - 1 : b;
    i0 = a; i1 = b;
    return x - fl;
}
template <bool SEQ>
__device__ __forceinline__ float4 sample_bilinear(const TexDev& t, float u, float v) {
    int x0, x1, y0, y1;
    float fx = unit_coord(u, t.w, x0, x1);
    float fy = unit_coord(v, t.h, y0, y1);
    float4 a = texel<SEQ>(t, x0, y0), b = texel<SEQ>(t, x1, y0), c = texel<SEQ>(t, x0, y1), d = texel<SEQ>(t, x1, y1);
    float4 r;
    r.x = mix_(mix_(a.x, b.x, fx), mix_(c.x, d.x, fx), fy);
    r.y = mix_(mix_(a.y, b.y, fx), mix_(c.y, d.y, fx), fy);
    r.z = mix_(mix_(a.z, b.z, fx), mix_(c.z, d.z, fx), fy);
    r.w = mix_(mix_(a.w, b.w, fx), mix_(c.w, d.w, fx), fy);
    return r;
}

// ------------------------------------------------------------------------------------------
// the accumulation's resolve (bhray_accum.hip, bhray_adapt.hip): a traced result as the colour that is summed
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

// sky.wgsl:19-26 without the store's binary16 rounding: sky_kernel's operations (bhray_kernels.hip)
__device__ __forceinline__ float4 resolve(const TexDev& sky, float4 p) {
    if (p.w == 0.0f) {
        const float theta = bh_atan2(sqrtf(p.x * p.x + p.z * p.z), p.y);
        const float phi = bh_atan2(p.z, p.x);
        const float PI_F = 3.1415926f;
        float u = (phi + 2.6f * PI_F) / (2.0f * PI_F);
        float v = (PI_F - theta) / PI_F;
        u = u - truncf(u); v = v - truncf(v);
        const float4 sc = sample_bilinear<false>(sky, u, v);
        p = make_float4((sc.x * sc.x) * (sc.x * sc.x), (sc.y * sc.y) * (sc.y * sc.y), (sc.z * sc.z) * (sc.z * sc.z), 1.0f);
    }
    return p;
}

}  // namespace bhray
