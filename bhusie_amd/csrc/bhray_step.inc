// bhray_step.inc - one integrator step of the lanes that are in M_REL (ray.wgsl:522-553), included by trace_kernel's step loop in
// one of two textual forms.  Both are the same operations on the same values; they differ in control flow only:
//   BHRAY_STEP_LEAN 0  the dense build (a saturated device): nested tests, `continue` on a disk hit, the step counted at the end of
//                      each arm - the form whose code generation the throughput numbers were measured with;
//   BHRAY_STEP_LEAN 1  the latency build (a wave alone on its SIMD pays ~30 cycles for every exec-mask region and join): ONE region per
//                      step - lanes that have used up their iterations leave through a select - and the step is counted before the
//                      rare-path branch (the rare paths that do not count it take it back), so the plain march has no else-arm:
//                      -9 % per iteration (level 0: 0.232 -> 0.201 ms).  The same form costs the dense build 0.6-1.2 % (A/B).
// (Written twice rather than parametrised: three attempts at one parametrised text changed the dense build's code.)
#if BHRAY_STEP_LEAN
            {
                const bool go = (mode == M_REL) & (it < H.max_iter);
                if ((mode == M_REL) & !go) mode = M_FINISH;
                if (go) {
                    if (COUNT) cnt[4]++;
                    ppos = cpos; pdir = cdir;
                    const float ppos_dist = cpos_dist;
                    float cd;
                    if (EVAL == 1) {
                        if (METHOD == 0) {
                            next_ray_euler_literal(bpos, cpos, cdir, H.step_size);
                        } else {
                            next_ray_rk_literal(bpos, rkpos, rkdir, rkh);
                            cpos = rkpos; cdir = rkdir;
                        }
                        cd = length_rn(cpos - bpos);                      // ray.wgsl:533, operator by operator
                    } else if (EVAL == 2) {
                        if (METHOD == 0) {
                            next_ray_euler_fma(bpos, cpos, cdir, H.step_size);
                        } else {
                            next_ray_rk_fma(bpos, rkpos, rkdir, rkh);
                            cpos = rkpos; cdir = rkdir;
                        }
                        cd = sqrt_rn(fdot(cpos - bpos, cpos - bpos));     // the integrator's distance with the fused dot
                    } else {
                    if (METHOD == 0) {
                        next_ray_euler(qrel, cpos, cdir, H.step_size, dist_c);
                    } else {
                        next_ray_rk<ERR_SKIP>(qrel, rkpos, rkdir, rkh, dist_c, cnt);
                        cpos = rkpos; cdir = rkdir;
                    }
                    qrel = cpos - bpos;
                    cd = sqrt_rn(fdot(qrel, qrel));               // N7: the integrator's distance (ray.wgsl:533) = fdistance(cpos, bpos)
                    }
                    dist_c = cd; cpos_dist = cd;                       // Euler: cpos is the integrator position; RK: cpos == rkpos here
                    closest = closest_min(cd, closest);
                    pdir = cdir;
                    // Everything that can end or alter the plain march - a horizon or disk test that is not culled, the sphere exit - sits
                    // behind ONE branch instead of the seven of the straightforward form (+2.5 % on a saturated device, measured; a wave
                    // that runs alone pays for every exec-mask region and join).  `amount` changes only in there, so does its test.
                    const float seg = METHOD == 0 ? H.step_size : rkh;
                    bool near_horizon, near_disk;
                    black_hole_culls<MODELS>(H, ppos, ppos_dist, seg, near_horizon, near_disk);
                    bool near_mesh = false;                          // lensed-mesh kernels only: may the segment touch a model? (lens_near_mesh)
                    if constexpr (LENSED) near_mesh = lens_near_mesh(P, ppos, pdir, seg);
                    it++;                                          // the plain march; the rare paths that do not count the step take it back
                    if (near_horizon || near_disk || cd > H.R || near_mesh) {
                    Hit crs; float td;
                    const bool disk = hit_black_hole_geom<PH>(H, ppos, pdir, near_horizon, near_disk, t_min, seg, crs, td);
                    if (cd > H.R) {
                        mode = M_FLAT;
                        const float fw = H.R * H.feather;
                        const float fs = H.R - fw;
                        const float lin = clamp_((closest - fs) / fw, 0.0f, 1.0f);
                        const float m = lin * lin;
                        cdir = mix3(cdir, cold.rdir(), m);
                    }
                    // Lensed meshes: hit_ray's models come after its black hole (ray.wgsl:369-389).  The lane pauses with ppos / pdir / seg (the uniform step, or rkh) and what
                    // the black hole's test found intact - none of the arms below is its own - and the lens phase traverses the models and merges in hit_ray's order
                    // (trace_kernel).  Both forms of this text count the step for such a lane (`it`); the lens phase takes that back first.
                    bool lens_paused = false;
                    if constexpr (LENSED) {
                        if (near_mesh) {
                            cold.set_pend_t(disk ? td : crs.t);
                            mode = lens_pause_mode(mode == M_FLAT, disk ? 2 : (crs.hit ? 1 : 0));
                            lens_paused = true;
                        }
                    }
                    if (disk && !lens_paused) {
                        // The shading of a disk hit (~700 instructions, needed by 1-5 lanes of a stepping wave) is deferred to the
                        // shade phase: the lane pauses with ppos / pdir / td intact and resumes in the mode it has now.
                        cold.set_pend_t(td);
                        mode = (mode == M_FLAT) ? M_SHADE_FLAT : M_SHADE_REL;
                        it--;                                    // the shade phase counts this step when the ray goes on
                    } else {
                    if (crs.hit && !lens_paused) {               // horizon: colour 0, opacity 1
                        cpos = cpos + pdir * crs.t;
                        cpos_dist = fdistance_ph<PH>(cpos, bpos);
                        if (METHOD == 0) { dist_c = cpos_dist; qrel = cpos - bpos; }
                        const F3 cc = f3(clamp_(crs.color.x, 0.0f, 1.0f), clamp_(crs.color.y, 0.0f, 1.0f), clamp_(crs.color.z, 0.0f, 1.0f));
                        cold.set_color(cold.color() + cc * (amount * crs.opacity));
                        amount *= 1.0f - crs.opacity;
                        if constexpr (RECORDS) { if (!HIT_GET()) record_first_hit(records, cold.pix(), cpos, (uint32_t)BHRAY_HIT_HORIZON, -1); }
                        HIT_SET(1);
                    }
                    if (amount < 0.005f) { mode = M_FINISH; it--; }
                    }
                    }
                    // PATHS: the count is final here - a lane that paused on the disk or finished took it back and left M_REL / M_FLAT; one that goes on (marching, or out of the sphere) keeps it
                    if constexpr (PATHS) { if ((mode == M_REL) | (mode == M_FLAT)) path_sample(path_points, cold.pix(), path_s, path_max, cpos, it); }
                }
            }
#else
            if (mode == M_REL) {
                if (it >= H.max_iter) {
                    mode = M_FINISH;
                } else {
                    if (COUNT) cnt[4]++;
                    ppos = cpos; pdir = cdir;
                    const float ppos_dist = cpos_dist;
                    float cd;
                    if (EVAL == 1) {
                        if (METHOD == 0) {
                            next_ray_euler_literal(bpos, cpos, cdir, H.step_size);
                        } else {
                            next_ray_rk_literal(bpos, rkpos, rkdir, rkh);
                            cpos = rkpos; cdir = rkdir;
                        }
                        cd = length_rn(cpos - bpos);                      // ray.wgsl:533, operator by operator
                    } else if (EVAL == 2) {
                        if (METHOD == 0) {
                            next_ray_euler_fma(bpos, cpos, cdir, H.step_size);
                        } else {
                            next_ray_rk_fma(bpos, rkpos, rkdir, rkh);
                            cpos = rkpos; cdir = rkdir;
                        }
                        cd = sqrt_rn(fdot(cpos - bpos, cpos - bpos));     // the integrator's distance with the fused dot
                    } else {
                    if (METHOD == 0) {
                        next_ray_euler(qrel, cpos, cdir, H.step_size, dist_c);
                    } else {
                        next_ray_rk<ERR_SKIP>(qrel, rkpos, rkdir, rkh, dist_c, cnt);
                        cpos = rkpos; cdir = rkdir;
                    }
                    qrel = cpos - bpos;
                    cd = sqrt_rn(fdot(qrel, qrel));               // N7: the integrator's distance (ray.wgsl:533) = fdistance(cpos, bpos)
                    }
                    dist_c = cd; cpos_dist = cd;                       // Euler: cpos is the integrator position; RK: cpos == rkpos here
                    closest = closest_min(cd, closest);
                    pdir = cdir;
                    // Everything that can end or alter the plain march - a horizon or disk test that is not culled, the sphere exit - sits
                    // behind ONE branch instead of the seven of the straightforward form (+2.5 % on a saturated device, measured; a wave
                    // that runs alone pays for every exec-mask region and join).  `amount` changes only in there, so does its test.
                    const float seg = METHOD == 0 ? H.step_size : rkh;
                    bool near_horizon, near_disk;
                    black_hole_culls<MODELS>(H, ppos, ppos_dist, seg, near_horizon, near_disk);
                    bool near_mesh = false;                          // lensed-mesh kernels only: may the segment touch a model? (lens_near_mesh)
                    if constexpr (LENSED) near_mesh = lens_near_mesh(P, ppos, pdir, seg);
                    if (near_horizon || near_disk || cd > H.R || near_mesh) {
                    Hit crs; float td;
                    const bool disk = hit_black_hole_geom<PH>(H, ppos, pdir, near_horizon, near_disk, t_min, seg, crs, td);
                    if (cd > H.R) {
                        mode = M_FLAT;
                        const float fw = H.R * H.feather;
                        const float fs = H.R - fw;
                        const float lin = clamp_((closest - fs) / fw, 0.0f, 1.0f);
                        const float m = lin * lin;
                        cdir = mix3(cdir, cold.rdir(), m);
                    }
                    // Lensed meshes: hit_ray's models come after its black hole (ray.wgsl:369-389).  The lane pauses with ppos / pdir / seg (the uniform step, or rkh) and what
                    // the black hole's test found intact - none of the arms below is its own - and the lens phase traverses the models and merges in hit_ray's order
                    // (trace_kernel).  Both forms of this text count the step for such a lane (`it`); the lens phase takes that back first.
                    bool lens_paused = false;
                    if constexpr (LENSED) {
                        if (near_mesh) {
                            cold.set_pend_t(disk ? td : crs.t);
                            mode = lens_pause_mode(mode == M_FLAT, disk ? 2 : (crs.hit ? 1 : 0));
                            lens_paused = true;
                        }
                    }
                    if (disk && !lens_paused) {
                        // The shading of a disk hit (~700 instructions, needed by 1-5 lanes of a stepping wave) is deferred to the
                        // shade phase: the lane pauses with ppos / pdir / td intact and resumes in the mode it has now.
                        cold.set_pend_t(td);
                        mode = (mode == M_FLAT) ? M_SHADE_FLAT : M_SHADE_REL;
                        continue;
                    }
                    if (crs.hit && !lens_paused) {               // horizon: colour 0, opacity 1
                        cpos = cpos + pdir * crs.t;
                        cpos_dist = fdistance_ph<PH>(cpos, bpos);
                        if (METHOD == 0) { dist_c = cpos_dist; qrel = cpos - bpos; }
                        const F3 cc = f3(clamp_(crs.color.x, 0.0f, 1.0f), clamp_(crs.color.y, 0.0f, 1.0f), clamp_(crs.color.z, 0.0f, 1.0f));
                        cold.set_color(cold.color() + cc * (amount * crs.opacity));
                        amount *= 1.0f - crs.opacity;
                        if constexpr (RECORDS) { if (!HIT_GET()) record_first_hit(records, cold.pix(), cpos, (uint32_t)BHRAY_HIT_HORIZON, -1); }
                        HIT_SET(1);
                    }
                    if (amount < 0.005f) mode = M_FINISH; else it++;
                    } else {
                        it++;
                    }
                    // PATHS: as above - a lane that paused on the disk has left through `continue`, one that finished was not counted and is in M_FINISH
                    if constexpr (PATHS) { if ((mode == M_REL) | (mode == M_FLAT)) path_sample(path_points, cold.pix(), path_s, path_max, cpos, it); }
                }
            }
#endif
