// bhray_quad_steps.inc - quad_march's batch of integrator steps (bhray_quad.inc), a file of its own for the same reason as bhray_march.inc: the round
// includes it behind the break test (BHRAY_PHASE_ORDER) or, the earlier order, behind the epilogue.
        // ---- a batch of integrator steps (bhray_step.inc's lean form, one component per lane)
        // (FrameLaunch::work is the GPU time of the march in units of a SCALAR wave's step - what bhray_rebalance balances: a quad wave's step is 150 of its
        // 207 instructions and 596 of its 832 clocks, so a batch of 16 counts as 12)
        if (__any(mode == M_REL)) work_steps += (unsigned)(BHRAY_REL_BATCH * 3 / 4);
        for (int k = 0; k < BHRAY_REL_BATCH; k++) {
            if (!__any(mode == M_REL)) break;
            const bool go = (mode == M_REL) & (it < H.max_iter);
            if ((mode == M_REL) & !go) mode = M_FINISH;
            if (go) {
                ppos = cpos; pdir = cdir;
                const float ppos_dist = cpos_dist;
                if (METHOD == 0) {
                    quad_euler(qrel, cpos, cdir, H.step_size, dist_c);
                } else {
                    quad_rk(qrel, rkpos, rkdir, rkh, dist_c);
                    cpos = rkpos; cdir = rkdir;
                }
                qrel = cpos - bh_c;
                const float cd = sqrt_rn(qdot_self(qrel));             // N7: the integrator's distance (ray.wgsl:533)
                dist_c = cd; cpos_dist = cd;
                if (cd < closest) closest = cd;
                pdir = cdir;
                const float seg = METHOD == 0 ? H.step_size : rkh;
                // black_hole_culls<false> on the quad: the plane distance is the one reduction
                const float numer = qdot_uniform(bh_c - ppos, H.bn);
                const float reach = 1.05f * seg + 0.05f;
                const bool near_horizon = ppos_dist <= 1.0f + reach;
                const bool near_disk = (ppos_dist <= H.outer + reach) & (fabsf(numer) <= (1.01f * seg) * H.bn_len + 1e-4f * H.bn_len);
                it++;
                if (near_horizon || near_disk || cd > H.R) {
                    Hit crs; float td;
                    const bool disk = hit_black_hole_geom<PHASE_SEQ_QUAD>(H, qgather(ppos), qgather(pdir), near_horizon, near_disk, t_min, seg, crs, td);
                    if (cd > H.R) {
                        mode = M_FLAT;
                        const float fw = H.R * H.feather;
                        const float fs = H.R - fw;
                        const float lin = clamp_((closest - fs) / fw, 0.0f, 1.0f);
                        const float m = lin * lin;
                        cdir = mix_(cdir, rdir_c, m);
                    }
                    if (disk) {
                        pend_t = td;
                        mode = (mode == M_FLAT) ? M_SHADE_FLAT : M_SHADE_REL;
                        it--;
                    } else {
                        if (crs.hit) {                                   // horizon: colour 0, opacity 1
                            cpos = cpos + pdir * crs.t;
                            cpos_dist = fdistance_ph<PHASE_SEQ_QUAD>(qgather(cpos), bpos);
                            if (METHOD == 0) { dist_c = cpos_dist; qrel = cpos - bh_c; }
                            const float cc = clamp_(qpick(crs.color, c), 0.0f, 1.0f);
                            col = col + cc * (amount * crs.opacity);
                            amount *= 1.0f - crs.opacity;
                            hit = 1;
                        }
                        if (amount < 0.005f) { mode = M_FINISH; it--; }
                    }
                }
            }
        }
