// bhray_march.inc - trace_kernel's march: one batch of integrator steps for the lanes inside the relativity sphere, with the iteration-limit test
// in front of the unified pairs and the state fix-up behind them.  A file of its own because the round includes it at one of two places
// (BHRAY_PHASE_ORDER, see the round's loop in bhray_kernels.hip): behind the refill, or - the earlier order - behind the epilogue.  One text, so both orders march alike.
        // ---- a batch of integrator steps (ray.wgsl:522-553) for lanes inside the sphere
        if (__any(mode == M_REL)) work_steps += (unsigned)REL_BATCH;
        if constexpr (UNIFIED) {
            // The unified march (bhray_step_u.inc): pairs of steps over two position register sets, the state that only the rare paths and the other
            // phases read (cpos / cdir / ppos / pdir apart from the integrator's own) written when a lane LEAVES the march, not on every step.
            // RK: the integrator runs on rkpos / rkdir and the hit test's segment starts at cpos, which differs from rkpos for one step after a
            // disk hit or a sphere entry moved it (ray.wgsl keeps two rays) - a wave that holds such a lane takes one step of the general form first.
            if (METHOD == 1) {
                const bool odd = (mode == M_REL) & ((cpos.x != rkpos.x) | (cpos.y != rkpos.y) | (cpos.z != rkpos.z) | (cpos_dist != dist_c));
                if (__any(odd)) {
                    work_steps += 1u;
                    {                                        // (the lean text in both builds: the dense text leaves a step with `continue`)
#define BHRAY_STEP_LEAN 1
#include "bhray_step.inc"
#undef BHRAY_STEP_LEAN
                    }
                }
            }
            if (mode == M_REL && it >= H.max_iter) mode = M_FINISH;      // the iteration limit (ray.wgsl:522) in front of the pairs; inside them it is tested where `it` changes
            F3& upos = METHOD == 0 ? cpos : rkpos;      // the integrator's position and direction
            F3& udir = METHOD == 0 ? cdir : rkdir;
            // (the hole at the origin - all three words +0 - marches without forming position - bpos: see bhray_step_u.inc.  A property of the BUILD, chosen by the host per launch: an
            // ORIGIN build holds the first loop only, every other build the second; BHRAY_ORIGIN_KERNEL 0, the earlier text: both loops in one kernel behind a wave-uniform scalar test)
#if BHRAY_ORIGIN_KERNEL
            if constexpr (ORIGIN) {
#else
            if (!MODELS && (BHRAY_ORIGIN_PATH & (1 << METHOD)) != 0 && ((__float_as_uint(H.bh.x) | __float_as_uint(H.bh.y) | __float_as_uint(H.bh.z)) == 0u)) {
#endif
#define BHRAY_U_ORIGIN 1
                for (int k = 0; k < REL_BATCH; k += 2) {
                    if (!__any(mode == M_REL)) break;
#define BHRAY_U_FIRST 1
#include "bhray_step_u.inc"
#undef BHRAY_U_FIRST
#define BHRAY_U_FIRST 0
#include "bhray_step_u.inc"
#undef BHRAY_U_FIRST
                }
                if (mode == M_REL) qrel = upos;
#undef BHRAY_U_ORIGIN
            } else {
#define BHRAY_U_ORIGIN 0
            for (int k = 0; k < REL_BATCH; k += 2) {
                if (!__any(mode == M_REL)) break;
#define BHRAY_U_FIRST 1
#include "bhray_step_u.inc"
#undef BHRAY_U_FIRST
#define BHRAY_U_FIRST 0
#include "bhray_step_u.inc"
#undef BHRAY_U_FIRST
            }
#undef BHRAY_U_ORIGIN
            }
            if (mode == M_REL) {                         // between batches every lane's state is exactly the general step's (after the second step of a pair ppos
                if (METHOD == 1) { cpos = rkpos; cdir = rkdir; }   // is the previous position already): a general step, the iteration limit inside it, the other phases read it
                pdir = udir;
                cpos_dist = dist_c;
            }
        } else {
        for (int k = 0; k < REL_BATCH; k++) {       // (unrolled by 2 / 4 to let prev = curr become renaming: -1 % / 0 %, measured)
            if (!__any(mode == M_REL)) break;
            if (COUNT && lane == 0) cnt[10]++;
            if (DENSE || MODELS) {                    // see bhray_step.inc
#define BHRAY_STEP_LEAN 0
#include "bhray_step.inc"
#undef BHRAY_STEP_LEAN
            } else {
#define BHRAY_STEP_LEAN 1
#include "bhray_step.inc"
#undef BHRAY_STEP_LEAN
            }
        }
        }
