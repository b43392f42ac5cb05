// bhray_quad.inc - the QUAD march: a thin launch's rays marched with the x, y, z components of ONE ray on three lanes of a quad
// (lane 4r + c holds component c of ray r of the wave's share; lane 4r + 3 carries a copy of z), instead of three registers of one lane.
//
// Why.  A launch whose queue is short lasts as long as its longest ray, and what that ray pays per iteration is the instruction stream of
// its wave - ~300 instructions of which ~150 are the Cash-Karp stages on 3-vectors, three instructions per vector operation - while 40 to
// 60 lanes of the wave hold nothing.  With one component per lane every 3-vector multiply / add / fma of ray.wgsl:401-480 is ONE
// instruction; what reduces over the components (the fused dots of h2, of the normalisation and of the exit distance, the cross product,
// e_max, the disk-plane distance of the culls) fetches its operands from the neighbouring lanes with quad_perm DPP moves IN THE SAME
// OPERATION ORDER - fdot = fma(z, z, fma(y, y, x * x)) and so on - so a ray is the same sequence of binary32 operations and every pixel
// the same bits (profiles/ubench/quad_xyz.hip: 832 -> 596 clocks per RK step for a wave alone on its SIMD, out[] identical; EXPERIMENTS.md R6.1).
// Everything that is rare - ray creation, a horizon / disk test that the culls let through, the sphere exit, disk shading, the flat-space
// iteration, the epilogue - gathers the ray's vectors into every lane of its quad (three DPP moves per vector) and runs the SAME device
// functions as trace_kernel, redundantly in the quad's lanes; lane c keeps component c of what comes back.
//
// Where.  The latency build of the no-mesh kernel under the numerics contract (EVAL == 0, not counting), for a frame whose queue fits
// 16 rays per wave on at most BHRAY_QUAD_MAX_WPS waves per SIMD; the rays are dealt out once, without an atomic, like the scalar thin
// shares (trace_kernel).  The host allows it per launch (TRACE_QUAD_WPS_* of FrameLaunch::trace_flags = waves per SIMD it may use; 0 = never).
#ifndef BHRAY_QUAD_MAX_WPS
#define BHRAY_QUAD_MAX_WPS 4
#endif

// quad_perm control words: lane i of a quad reads lane sel[i] of the same quad
#define BHRAY_QP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
template <int CTRL> __device__ __forceinline__ float qperm(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float qx(float v) { return qperm<BHRAY_QP(0, 0, 0, 0)>(v); }     // component x of the quad's ray, in every lane of the quad
__device__ __forceinline__ float qy(float v) { return qperm<BHRAY_QP(1, 1, 1, 1)>(v); }
__device__ __forceinline__ float qz(float v) { return qperm<BHRAY_QP(2, 2, 2, 2)>(v); }
__device__ __forceinline__ float qr1(float v) { return qperm<BHRAY_QP(1, 2, 0, 0)>(v); }    // component c + 1 (cyclic); lane 3 follows lane 2
__device__ __forceinline__ float qr2(float v) { return qperm<BHRAY_QP(2, 0, 1, 1)>(v); }    // component c + 2
__device__ __forceinline__ F3 qgather(float v) { return f3(qx(v), qy(v), qz(v)); }            // the whole vector, in every lane of the quad
__device__ __forceinline__ float qpick(F3 v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : v.z); }   // (lane 3: z)
// fdot(a, a) (bhray_math.h): fma(a.z, a.z, fma(a.y, a.y, a.x * a.x)), in every lane of the quad
__device__ __forceinline__ float qdot_self(float a) {
    const float p = a * a;
    const float ay = qy(a), az = qz(a);
    return fmaf(az, az, fmaf(ay, ay, qx(p)));
}
// fdot(a, u) with a wave-uniform u
__device__ __forceinline__ float qdot_uniform(float a, F3 u) { return fmaf(qz(a), u.z, fmaf(qy(a), u.y, qx(a) * u.x)); }
// fcross(a, b).c = fma(a[c+1], b[c+2], -(a[c+2] * b[c+1]))
__device__ __forceinline__ float qcross(float a, float b) { return fmaf(qr1(a), qr2(b), -(qr2(a) * qr1(b))); }

// next_ray_rk (above), one component per lane: q0, pos, dir are this lane's components; h_io, dist the ray's, in every lane of its quad
__device__ __forceinline__ void quad_rk(float q0, float& pos, float& dir, float& h_io, float dist) {
    const float p0 = pos, d0 = dir;
    const float cr = qcross(p0, d0);
    const float h2 = qdot_self(cr);
    const float s = (-1.5f * h2) * rcp_rn(pow5(dist));
    const float h = h_io, sh = s * h;
    const float K1 = q0 * sh;
    const float K2 = fmaf(K1, A21, q0) * sh;
    const float K3 = fmaf(K2, A32, fmaf(K1, A31, q0)) * sh;
    const float K4 = fmaf(K2, A43, fmaf(K2, A42, fmaf(K1, A41, q0))) * sh;
    const float K5 = fmaf(K4, A54, fmaf(K3, A53, fmaf(K2, A52, fmaf(K1, A51, q0)))) * sh;
    const float K6 = fmaf(K5, A65, fmaf(K4, A64, fmaf(K3, A63, fmaf(K2, A62, fmaf(K1, A61, q0))))) * sh;
    const float e = fmaf(K6, DB6, fmaf(K5, DB5, fmaf(K4, DB4, fmaf(K3, DB3, K1 * DB1))));
    const float ae = fabsf(e);
    const float e_max = max_(max_(qx(ae), qy(ae)), qz(ae));
    const float ds = fmaf(K6, BA6, fmaf(K5, BA5, fmaf(K4, BA4, fmaf(K3, BA3, K1 * BA1))));
    const float a = d0 + ds;
    const float d = qdot_self(a);                                  // fnormalize_rn
    float r = rcp_newton(sqrt_corrected(d));
    if (__builtin_expect(__ballot(!sqrt_in_range(d)) != 0ull, 0)) r = 1.0f / sqrtf(d);
    dir = a * r;
    pos = fmaf(d0, h, p0);
    if (e_max > 0.00002f) h_io = h * (0.9f * pow_m001_step(e_max));
    else h_io = h * 1.0001f;
}
// next_ray_euler (above), one component per lane
__device__ __forceinline__ void quad_euler(float q0, float& pos, float& dir, float step, float dist) {
    const float cr = qcross(pos, dir);
    const float h2 = qdot_self(cr);
    const float s = (-1.5f * h2) * rcp_rn(pow5(dist));
    const float a = fmaf(q0, s * step, dir);
    const float d = qdot_self(a);                                  // fnormalize_rn
    float r = rcp_newton(sqrt_corrected(d));
    if (__builtin_expect(__ballot(!sqrt_in_range(d)) != 0ull, 0)) r = 1.0f / sqrtf(d);
    dir = a * r;
    pos = fmaf(dir, step, pos);
}

// The rays [first, first + count * stride) of the frame's queue (stride 0: consecutive entries) marched by this wave, ray r on quad r.
// Same phases as trace_kernel's loop on the same values, in its order (BHRAY_PHASE_ORDER: a batch of steps, shade, flat, epilogue; 0: the batch last); see the file header.
template <int METHOD>
__device__ __forceinline__ void quad_march(const FrameParams& P, const FrameLaunch& F, const HotParams& H, const uint32_t qcount,
                                           const uint32_t first, const uint32_t count, const uint32_t stride, unsigned& work_steps) {
    const LevelParams& L = F.L;
    const SpecLevels& SL = F.SL;
    const int lane = (int)lanes_below(~0ull);
    const int c = lane & 3;
    const uint32_t r = (uint32_t)lane >> 2;
    const F3 bpos = H.bh;
    const float bh_c = qpick(H.bh, c);
    const float t_max = 1e5f, t_min = 1e-8f;

    int mode = M_EMPTY, it = 0, hit = 0;
    uint32_t pix = 0;
    float cpos = 0.0f, cdir = 0.0f, ppos = 0.0f, pdir = 0.0f, rkpos = 0.0f, rkdir = 0.0f, qrel = 0.0f, col = 0.0f, rdir_c = 0.0f;
    float rkh = 0.0f, amount = 1.0f, closest = H.ray_distance, dist_c = P.ray_distance_f, cpos_dist = P.ray_distance_f, pend_t = 0.0f;

    // ---- this wave's share, once (create_ray, ray.wgsl:269-285: as trace_kernel's refill)
    {
        const uint32_t idx = stride != 0u ? first + r * stride : first + r;
        if (r < count && idx < qcount) {
            pix = F.queue[idx];
            const int px = (int)(pix & 0x7fffu), py = (int)((pix >> 15) & 0x7fffu);
            int lw = L.w, lh = L.h;
            if (SL.n > 0) {
                const int lv = (int)(pix >> 30);
                lw = SL.l[0].w; lh = SL.l[0].h;
#pragma unroll
                for (int q = 1; q < BHRAY_MAX_SPEC_LEVELS; q++) if (lv == q) { lw = SL.l[q].w; lh = SL.l[q].h; }
            }
            const int sm = (lw - 1) < (lh - 1) ? (lw - 1) : (lh - 1);
            const float increment = 1.0f / (float)sm;
            const float posx = (2.0f * ((float)px - (float)(lw - 1) * 0.5f)) * increment;
            const float posy = (2.0f * ((float)py - (float)(lh - 1) * 0.5f)) * increment;
            const F3 cam = ld3(P.cam);
            const F3 rdir = normalize((ld3(P.right) * posx + ld3(P.up) * posy) + ld3(P.fwd_ff));
            const float cam_c = qpick(cam, c);
            rdir_c = qpick(rdir, c);
            cpos = cam_c; cdir = rdir_c; ppos = cam_c; pdir = rdir_c;
            rkpos = cam_c; rkdir = rdir_c; rkh = P.step_size;
            col = 0.0f; amount = 1.0f; closest = H.ray_distance;
            dist_c = P.ray_distance_f; cpos_dist = P.ray_distance_f; qrel = cam_c - bh_c;
            it = 0; hit = 0;
            mode = P.relativity0 ? M_REL : M_FLAT;
        }
    }

    for (;;) {
        if (!__any(mode != M_EMPTY)) break;
#if BHRAY_PHASE_ORDER
#include "bhray_quad_steps.inc"
#endif
        // ---- deferred disk shading (as trace_kernel)
        if (__any(mode >= M_SHADE_REL)) {
            if (mode >= M_SHADE_REL) {
                Hit crs; crs.hit = true; crs.t = pend_t; crs.color = f3(0.0f, 0.0f, 0.0f); crs.opacity = 0.0f;
                shade_disk<false, PHASE_SEQ_QUAD, POW13_QUAD>(H, qgather(ppos), qgather(pdir), pend_t, H.ray_distance, crs, nullptr);
                cpos = cpos + pdir * crs.t;
                cpos_dist = fdistance_ph<PHASE_SEQ_QUAD>(qgather(cpos), bpos);
                if (METHOD == 0) { dist_c = cpos_dist; qrel = cpos - bh_c; }
                const float cc = clamp_(qpick(crs.color, c), 0.0f, 1.0f);
                col = col + cc * (amount * crs.opacity);
                amount *= 1.0f - crs.opacity;
                hit = 1;
                if (amount < 0.005f) mode = M_FINISH;
                else { it++; mode = (mode == M_SHADE_FLAT) ? M_FLAT : M_REL; }
            }
        }
        // ---- flat-space iterations (ray.wgsl:554-569; no meshes in this build: the sphere alone)
        if (__any(mode == M_FLAT)) {
            if (mode == M_FLAT) {
                if (it >= H.max_iter) {
                    mode = M_FINISH;
                } else {
                    float ths = t_max;
                    const bool hs = hit_sphere<PHASE_SEQ_QUAD>(qgather(ppos), qgather(pdir), H.R, bpos, t_min, t_max, ths);
                    if (!hs) {
                        mode = M_FINISH;                                   // break (no increment)
                    } else {                                               // (the sphere is always nearer than "no mesh hit": ths < t_max)
                        cpos = cpos + cdir * ths; mode = M_REL;
                        cpos_dist = fdistance_ph<PHASE_SEQ_QUAD>(qgather(cpos), bpos);
                        if (METHOD == 0) { dist_c = cpos_dist; qrel = cpos - bh_c; }
                        if (amount < 0.005f) mode = M_FINISH; else it++;
                    }
                }
            }
        }
        // ---- epilogue (ray.wgsl:583-595)
        if (__any(mode == M_FINISH)) {
            if (mode == M_FINISH) {
                float4 o;
                F3 color = qgather(col);
                const F3 cd3 = qgather(cdir);
                if (hit != 0 || it <= 5) {
                    if (amount > 0.001f) {
                        const float theta = bh_atan2(sqrtf(cd3.x * cd3.x + cd3.z * cd3.z), cd3.y);
                        const float phi = bh_atan2(cd3.z, cd3.x);
                        const float PI_F = 3.1415926f;
                        float u = (phi + 2.6f * PI_F) / (2.0f * PI_F);
                        float v = (PI_F - theta) / PI_F;
                        u = u - truncf(u); v = v - truncf(v);
                        const float4 sc = sample_bilinear<PHASE_SEQ_QUAD>(P.sky, u, v);
                        const F3 miss = f3((sc.x * sc.x) * (sc.x * sc.x), (sc.y * sc.y) * (sc.y * sc.y), (sc.z * sc.z) * (sc.z * sc.z));
                        color = color + miss * amount;
                    }
                    o = make_float4(color.x, color.y, color.z, 1.0f);
                } else {
                    o = make_float4(cd3.x, cd3.y, cd3.z, 0.0f);
                }
                if (c == 0) {                                              // one lane of the quad stores
                    const int ox = (int)(pix & 0x7fffu), oy = (int)((pix >> 15) & 0x7fffu);
                    if (SL.n > 0) {
                        const int lv = (int)(pix >> 30);
                        float4* dst = SL.l[0].out; int pitch = SL.l[0].out_pitch, x0 = SL.l[0].out_x0; const int32_t* rowmap = SL.l[0].rowmap;
#pragma unroll
                        for (int q = 1; q < BHRAY_MAX_SPEC_LEVELS; q++) if (lv == q) { dst = SL.l[q].out; pitch = SL.l[q].out_pitch; x0 = SL.l[q].out_x0; rowmap = SL.l[q].rowmap; }
                        const int orow = rowmap ? rowmap[oy] : oy;
                        dst[(size_t)orow * (size_t)pitch + (size_t)(ox - x0)] = o;
                        if (F.stamp_value != 0u) {
                            uint32_t* st = SL.l[0].stamp; int sw = SL.l[0].w;
#pragma unroll
                            for (int q = 1; q < BHRAY_MAX_SPEC_LEVELS; q++) if (lv == q) { st = SL.l[q].stamp; sw = SL.l[q].w; }
                            st[(size_t)oy * (size_t)sw + (size_t)ox] = F.stamp_value;
                        }
                    } else {
                        L.out[out_index(L, ox, oy)] = o;
                    }
                }
                mode = M_EMPTY;
            }
        }
#if !BHRAY_PHASE_ORDER
#include "bhray_quad_steps.inc"
#endif
    }
}
