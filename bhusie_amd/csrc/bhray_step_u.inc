// bhray_step_u.inc - one integrator step of the UNIFIED march (round 6), included twice by trace_kernel's pair loop: BHRAY_U_FIRST 1, then 0.
//
// The general step (bhray_step.inc) keeps six 3-vectors per lane - cpos / cdir (the ray the hit tests see), ppos / pdir (the step's segment), rkpos / rkdir
// (the Cash-Karp integrator's own ray: ray.wgsl:405-465 keeps two) - and after a plain step four of them are copies: 16 `v_mov` of ~195 vector instructions.
// A lane that MARCHES needs three: the position before the step (the segment's start), the position after it, the direction.  Here a pair of steps
// alternates two position register sets - the first step reads `upos` (rkpos / Euler: cpos) and writes `ppos`, the second reads `ppos` and writes `upos` -
// the direction is updated in place, and the other vectors are written once, when a lane LEAVES the march (a disk hit, the horizon, the sphere's
// surface, the iteration limit): the state every other phase finds is exactly the general step's.  Same operations on the same values in the same
// order per ray: byte-identical frames (tests/test_gpu_step_forms.py and every parity test: these are the kernels that ship).
//
// Invariant at the head of a pair for a lane in M_REL: upos / udir = the integrator's ray, qrel = upos - bpos, dist_c = |qrel| = cpos_dist; RK: cpos == rkpos
// (a wave with a lane for which that does not hold takes one general step first: trace_kernel).  INSIDE a pair ppos / pdir / cpos_dist (RK: cpos, cdir) of a
// marching lane are not current; trace_kernel writes them behind the last pair, so that between batches every lane's state is exactly the general step's.
#if BHRAY_U_FIRST
#define U_PIN upos
#define U_POUT ppos
#else
#define U_PIN ppos
#define U_POUT upos
#endif
// BHRAY_U_ORIGIN 1: the hole sits at the scene's origin (the reference's default, blackhole.rs:16; all three words +0): position - bpos IS the position, bit for bit
// (x - (+0) = x for every x, -0 and NaN included), so the hole-relative vector is not formed per step; `qrel` is written when a lane leaves and behind the last pair.
#if BHRAY_U_ORIGIN
#define U_QIN U_PIN
#define U_QOUT U_POUT
#else
#define U_QIN qrel
#define U_QOUT qrel
#endif
#ifdef BHRAY_SHARE_LOG
#define U_SLOG , slog
#else
#define U_SLOG
#endif
            {
                // (The iteration limit, ray.wgsl:522, is tested where `it` changes - behind the step, in the rare-path test - and once in front of the pairs:
                // a lane in M_REL here has iterations left.)
                const bool go = mode == M_REL;
                if (go) {
                    const float pdist = dist_c;                              // |segment start - bpos| (the general step's ppos_dist)
                    float pnumer = fdot(U_QIN, H.bn);
                    // Euler: formed HERE, between the step's first multiplies - not sunk to the culls, where its three scalar operands would sit next to the compares' (instructions that
                    // touch the scalar register file issue at half rate next to each other, EXPERIMENTS.md R6.9): +0.8 %; the RK kernel loses 0.4 % to the extra live register
                    if (METHOD == 0 && BHRAY_PNUMER_EARLY) asm volatile("" : "+v"(pnumer));                  // the culls' plane distance of the segment's start, from the hole-relative position the integrator carries
                    // ONE_TEST: the step with the short sequences and nothing else (no range tests, no step-size power); `redo` = the lanes for which that is not the
                    // exact step - they run it again, exactly, behind the rare-path test, from the direction / step size / closest approach saved here
                    const F3 d0s = udir; const float hs = rkh, cls = closest;
                    bool redo = false;
                    float cd;
                    if (ONE_TEST) {
                        if (METHOD == 0) redo = next_ray_euler_t<true>(U_QIN, U_PIN, U_POUT, udir, H.step_size, dist_c);
                        else redo = next_ray_rk_t<true, ERR_SKIP>(U_QIN, U_PIN, U_POUT, udir, rkh, dist_c U_SLOG);
                        if (!BHRAY_U_ORIGIN) qrel = U_POUT - bpos;
                        const float qq = fdot(U_QOUT, U_QOUT);
                        cd = sqrt_corrected(qq);
                        redo |= !sqrt_in_range(qq);
                        if (BHRAY_ONE_TEST & 4) redo |= ((((unsigned)it * 2654435761u) ^ (cold.pix() * 40503u)) & 0x1c0u) == 0u;     // (test build: an eighth of the steps)
                    } else {
                        if (METHOD == 0) next_ray_euler_to(U_QIN, U_PIN, U_POUT, udir, H.step_size, dist_c);
                        else (void)next_ray_rk_t<false, ERR_SKIP>(U_QIN, U_PIN, U_POUT, udir, rkh, dist_c U_SLOG);
                        if (!BHRAY_U_ORIGIN) qrel = U_POUT - bpos;
                        cd = sqrt_rn(fdot(U_QOUT, U_QOUT));                 // N7: the integrator's distance (ray.wgsl:533)
                    }
                    dist_c = cd;
                    closest = closest_min(cd, closest);
                    float seg = METHOD == 0 ? H.step_size : rkh;
                    bool near_horizon, near_disk;
                    black_hole_culls_rel<MODELS>(H, pnumer, pdist, seg, near_horizon, near_disk);
                    it++;                                                   // the plain march; the rare paths that do not count the step take it back
                    if (near_horizon || near_disk || cd > H.R || it >= H.max_iter || redo) {
                        if (ONE_TEST) {
                            if (redo) {                                     // the exact step, from the same operands (qrel of the segment's start is U_PIN - bpos again, bit for bit)
                                udir = d0s; closest = cls;
                                if (METHOD == 1) rkh = hs;
                                const F3 q0 = U_PIN - bpos;
                                if (METHOD == 0) next_ray_euler_to(q0, U_PIN, U_POUT, udir, H.step_size, pdist);
                                else next_ray_rk_to(q0, U_PIN, U_POUT, udir, rkh, pdist);
                                if (!BHRAY_U_ORIGIN) qrel = U_POUT - bpos;
                                cd = sqrt_rn(fdot(U_QOUT, U_QOUT));
                                dist_c = cd;
                                closest = closest_min(cd, closest);
                                seg = METHOD == 0 ? H.step_size : rkh;
                                black_hole_culls_rel<MODELS>(H, pnumer, pdist, seg, near_horizon, near_disk);
                            }
                        }
#ifdef BHRAY_SHARE_LOG
                        if (slog) {
                            const unsigned long long active = __ballot(true), heavy_m = __ballot(near_horizon || near_disk || redo);
                            if ((int)(threadIdx.x & 63u) == (int)__builtin_ctzll(active)) { slog[2]++; if (heavy_m == 0ull) slog[3]++; }
                        }
#endif
                        // (A wave whose lanes here only leave the sphere or end at the iteration limit does not run the hit tests: the compiler branches round hit_sphere,
                        // hit_torus2d, the horizon arm and the disk arm when no lane takes them.  An arm of its own for such waves was built and lost 1.3 %: EXPERIMENTS.md R19.1.)
                        Hit crs; float td;
                        const bool disk = hit_black_hole_geom<PH>(H, U_PIN, udir, near_horizon, near_disk, t_min, seg, crs, td);
                        F3 ncpos = U_POUT, ncdir = udir;                    // what cpos / cdir become for a lane that leaves
                        float ncd = cd;
                        if (cd > H.R) {
                            mode = M_FLAT;
                            const float fw = H.R * H.feather;
                            const float fs = H.R - fw;
                            const float lin = clamp_((closest - fs) / fw, 0.0f, 1.0f);
                            const float m = lin * lin;
                            ncdir = mix3(udir, cold.rdir(), m);
                        }
                        if (disk) {
                            cold.set_pend_t(td);                            // shaded in the shade phase (see bhray_step.inc); the lane resumes in the mode it has now
                            mode = (mode == M_FLAT) ? M_SHADE_FLAT : M_SHADE_REL;
                            it--;
                        } else {
                            if (crs.hit) {                                  // horizon: colour 0, opacity 1
                                ncpos = ncpos + udir * crs.t;
                                ncd = fdistance_ph<PH>(ncpos, bpos);
                                if (METHOD == 0) { dist_c = ncd; if (!BHRAY_U_ORIGIN) qrel = ncpos - bpos; }
                                const F3 cc = f3(clamp_(crs.color.x, 0.0f, 1.0f), clamp_(crs.color.y, 0.0f, 1.0f), clamp_(crs.color.z, 0.0f, 1.0f));
                                cold.set_color(cold.color() + cc * (amount * crs.opacity));
                                amount *= 1.0f - crs.opacity;
                                if constexpr (RECORDS) { if (!HIT_GET()) record_first_hit(records, cold.pix(), ncpos, (uint32_t)BHRAY_HIT_HORIZON, -1); }
                                HIT_SET(1);
                            }
                            if (amount < 0.005f) { mode = M_FINISH; it--; }
                        }
                        if (mode == M_REL && it >= H.max_iter) mode = M_FINISH;      // what the next step's first test would find (the general step's state is the same there)
                        if (mode != M_REL) {                                // the lane leaves the march: the general step's state, in the general step's registers
                            const F3 p0 = U_PIN, p1 = U_POUT, d1 = udir;
                            ppos = p0; pdir = d1;
                            if (METHOD == 1) rkpos = p1;
                            cpos = ncpos; cdir = ncdir;
                            cpos_dist = ncd;
                            if (BHRAY_U_ORIGIN) qrel = METHOD == 0 ? ncpos : p1;      // = integrator position - bpos
                        }
                    }
                }
            }
#undef U_PIN
#undef U_POUT
#undef U_QIN
#undef U_QOUT
#undef U_SLOG
