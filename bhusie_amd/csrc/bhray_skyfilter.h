// bhray_skyfilter.h — the footprint-filtered sky pass (bhray_set_sky_filter): what the engine (bhray_api.hip) passes to the kernels of bhray_skyfilter.hip.
#pragma once
#include "bhray_internal.h"
#include "bhray_math.h"

namespace bhray {

// A texture side is at most 32768 = 2^15 (dev_set_texture): levels 0 .. 15.
constexpr int SKY_PYR_MAX_LEVELS = 16;

// The pyramid above the RGBA8 texture: levels 1 .. levels - 1 in one allocation, level after level, a texel four binary16 (r, g, b, 1.0).
struct SkyPyr {
    const uint2* base;                    // nullptr: a 1 x 1 texture has no level above it
    uint32_t off[SKY_PYR_MAX_LEVELS];     // first texel of level l in base (off[0] is not used)
    int levels;                           // level 0 included
};
// side of level l of a side of n texels: l times (n + 1) >> 1, which is ceil(n / 2^l)
BH_HD int sky_pyr_dim(int n, int l) { return (int)(((unsigned)n + (1u << l) - 1u) >> l); }

// bhray_sky_pyramid_sizes: lw / lh need room for 32 entries
int sky_pyramid_sizes(uint32_t w, uint32_t h, uint32_t* levels, uint32_t* lw, uint32_t* lh);
// SkyPyr::off / levels of a w x h texture (base stays nullptr); returns the texels of levels 1 .. top
size_t sky_pyramid_layout(int w, int h, SkyPyr* out);
// level 1 from the RGBA8 texture's radiance ((b / 255)^4, the sky pass's power); level l + 1 from the stored halves of level l.  One thread per written texel.  Enqueue only.
hipError_t launch_sky_pyramid_first(const TexDev& sky, uint2* dst, hipStream_t s);
hipError_t launch_sky_pyramid_next(const uint2* src, int sw, int sh, uint2* dst, hipStream_t s);
// the filtered sky pass over a whole frame_w x frame_h RGBA32F frame -> RGBA16F.  Enqueues only.
hipError_t launch_sky_filter(const TexDev& sky, const SkyPyr& pyr, const float4* src, uint2* dst_rgba16f, uint32_t frame_w, uint32_t frame_h, hipStream_t s);

}  // namespace bhray
