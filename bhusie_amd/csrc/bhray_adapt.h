// bhray_adapt.h — adaptive stills (bhray_accum_add_adaptive): what the engine (bhray_api.hip) passes to the kernels of bhray_adapt.hip.
#pragma once
#include "bhray_accum.h"

namespace bhray {

// A pixel's adaptive state beside its sum, one 16-byte word: x = S1 and y = S2 as binary32 bits (the sums of the compressed luminance t and of t * t), z = issued
// (sample indices given to the pixel), w = 0.  All zero after bhray_accum_begin.
//
// The test (include/bhray.h), one rounded binary32 operation each: n = sum.w, m = S1 / n, q = S2 / n, v = q - m * m, v = v < 0 ? 0 : v, e = tolerance * (m + dark);
// converged iff v <= (e * e) * n (false for a NaN, so for n == 0).

// ctl[0] = 0, ctl[1] = 0 before the launch (the caller clears them in stream order).  Behind it: ctl[0] pixels p with issued[p] < max_samples that are not converged, their
// indices in list[0 .. ctl[0]) - ascending within a block, the blocks in any order -, ctl[1] the largest issued among them.  list holds npix words.  Enqueues only.
hipError_t launch_adapt_select(const float4* sum, const uint4* state, uint32_t npix, uint32_t max_samples, float tolerance, float dark, uint32_t* list, uint32_t* ctl,
                               hipStream_t s);
// records jj * n_active + i of `rays` (two float4 each), jj = 0 .. g.k - 1, i = 0 .. n_active - 1: the ray of sample issued[p] + j0 + jj through frame pixel p = list[i]
// (list == nullptr: p = i), by accum_gen_kernel's operations.  g.s0 is not read.  g.k * n_active <= 2^26.  Enqueues only.
hipError_t launch_adapt_gen(const AccumGen& g, const uint32_t* list, uint32_t n_active, uint32_t j0, const uint4* state, float4* rays, hipStream_t s);
// pixel p = list[i] (nullptr: i) takes results[jj * n_active + i], jj = 0 .. k - 1 in that order, by the rule of include/bhray.h: resolve, skip what is not finite,
// sum += (r, g, b, 1), S1 += t, S2 += t * t.  advance: added to issued[p] (the round's sample count behind its last chunk, 0 behind the others).  A pixel occurs once
// in a list, so there is one writer per word.  Enqueues only.
hipError_t launch_adapt_add(const TexDev& sky, const float4* results, const uint32_t* list, uint32_t n_active, uint32_t k, uint32_t advance, float4* sum, uint4* state,
                            hipStream_t s);
// counts[p] = issued[p].  Enqueues only.
hipError_t launch_adapt_counts(const uint4* state, uint32_t* counts, uint32_t npix, hipStream_t s);

}  // namespace bhray
