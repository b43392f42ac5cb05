// bhray_accum_stars.h — point stars in stills (bhray_accum_set_stars): the catalogue of bhray_set_stars lensed into every sample image of the
// accumulation.  What the engine (bhray_api.hip) passes to the kernel of bhray_accum_stars.hip.  The rule is §23's - star_corner and star_pixel of bhray_stars.h,
// unchanged and shared with star_kernel - over a sample's trace results as "the frame".
#pragma once
#include "bhray_stars.h"

namespace bhray {

// T[j * npix + p] for j = 0 .. k - 1 and every frame pixel p: results[j * npix + p] bit for bit, except where the pixel accepted a star under §23's rules 1 - 6 over
// sample j's own frame_w x frame_h image (wrap_x != 0: periodic in x, column -1 is column frame_w - 1 and column frame_w is column 0); there
// (min(b.x + acc.x * gain, 65504.0f), .., .., 1.0f), b the accumulation's resolve (binary32 sky^4) of the pixel.  T must not overlap results.  Enqueues only.
hipError_t launch_accum_stars(const StarSet& S, const TexDev& sky, const float4* results, float4* T, uint32_t frame_w, uint32_t frame_h, uint32_t k, int wrap_x, hipStream_t s);

}  // namespace bhray
