// bhray_stars.h — point stars (bhray_set_stars): a star catalogue lensed into the sky pass.  What the engine (bhray_api.hip) passes to the kernel of
// bhray_stars.hip, and the two functions - star_corner and star_pixel - that are the rule of §23 on the device and on the host (bhray_stars_resolve_host): binary32, one
// rounded operation at a time (the TUs are compiled -ffp-contract=off), + - * / sqrt and compares only.
#pragma once
#include <vector>

#include "bhray_internal.h"
#include "bhray_math.h"

struct bhray_star_pixel_info;  // include/bhray_diag.h

namespace bhray {

// The catalogue as the kernel reads it: the stars sorted by (cell, original index), two float4 each - (dir.xyz, 0), (flux.rgb, 0) -, and the cells' prefix array
// (6 G G + 1 entries: the stars of cell k are prefix[k] .. prefix[k + 1] - 1).  Device pointers in the kernel's copy, host pointers in bhray_stars_resolve_host's.
struct StarSet {
    const float4* stars;
    const uint32_t* prefix;
    uint32_t G;                // cells per side of a cube face, a power of two in [1, 1024]
    float gain, min_area;
    float max_fp2;             // max_footprint * max_footprint
};

BH_HD bool star_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
BH_HD bool star_dir_pixel(float4 p) { return p.w == 0.0f && star_finite(p.x) && star_finite(p.y) && star_finite(p.z); }

// §23.1: the corner between four pixels (d00 above left, d10 above right, d01 below left, d11 below right); false: not valid
BH_HD bool star_corner(float4 d00, float4 d10, float4 d01, float4 d11, F3& c) {
    c = ((f3(d00.x, d00.y, d00.z) + f3(d10.x, d10.y, d10.z)) + (f3(d01.x, d01.y, d01.z) + f3(d11.x, d11.y, d11.z))) * 0.25f;
    return star_dir_pixel(d00) && star_dir_pixel(d10) && star_dir_pixel(d01) && star_dir_pixel(d11);
}

// §23.4: face 0 .. 5 = +x -x +y -y +z -z of the largest |component| (ties: x, then y); (a, b) = the other two components, in x y z order, over that magnitude
BH_HD uint32_t star_face(F3 d, float& a, float& b) {
    const float ax = d.x < 0.0f ? -d.x : d.x, ay = d.y < 0.0f ? -d.y : d.y, az = d.z < 0.0f ? -d.z : d.z;
    if (ax >= ay && ax >= az) { a = d.y / ax; b = d.z / ax; return d.x < 0.0f ? 1u : 0u; }
    if (ay >= az) { a = d.x / ay; b = d.z / ay; return d.y < 0.0f ? 3u : 2u; }
    a = d.x / az; b = d.y / az; return d.z < 0.0f ? 5u : 4u;
}
// floorf((a * 0.5f + 0.5f) * G) clamped to [0, G - 1]; the compares come before the conversion, so no value of a is undefined
BH_HD uint32_t star_cell_coord(float a, uint32_t G) {
    const float t = floorf((a * 0.5f + 0.5f) * (float)G);
    if (!(t >= 0.0f)) return 0u;
    if (t > (float)(G - 1u)) return G - 1u;
    return (uint32_t)t;
}
BH_HD uint32_t star_cell_of(F3 d, uint32_t G) {
    float a, b;
    const uint32_t f = star_face(d, a, b);
    return (f * G + star_cell_coord(b, G)) * G + star_cell_coord(a, G);
}

// the cell box of a footprint on face f: false when the face is not visited (a corner without a positive component along it, or a box that misses the face)
BH_HD bool star_face_box(uint32_t f, F3 c00, F3 c10, F3 c01, F3 c11, uint32_t G, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) {
    const uint32_t axis = f >> 1;
    const float sgn = (f & 1u) ? -1.0f : 1.0f;
    float m[4], a[4], b[4];
    const F3 c[4] = {c00, c10, c01, c11};
    for (int i = 0; i < 4; i++) {
        m[i] = (axis == 0 ? c[i].x : axis == 1 ? c[i].y : c[i].z) * sgn;
        a[i] = axis == 0 ? c[i].y : c[i].x;
        b[i] = axis == 2 ? c[i].y : c[i].z;
    }
    if (!(m[0] > 0.0f && m[1] > 0.0f && m[2] > 0.0f && m[3] > 0.0f)) return false;
    for (int i = 0; i < 4; i++) { a[i] = a[i] / m[i]; b[i] = b[i] / m[i]; }
    const float EPS = 0x1p-12f;
    const float alo = min_(min_(a[0], a[1]), min_(a[2], a[3])) - EPS, ahi = max_(max_(a[0], a[1]), max_(a[2], a[3])) + EPS;
    const float blo = min_(min_(b[0], b[1]), min_(b[2], b[3])) - EPS, bhi = max_(max_(b[0], b[1]), max_(b[2], b[3])) + EPS;
    if (!(alo <= 1.0f && ahi >= -1.0f && blo <= 1.0f && bhi >= -1.0f)) return false;
    a0 = star_cell_coord(alo, G); a1 = star_cell_coord(ahi, G);
    b0 = star_cell_coord(blo, G); b1 = star_cell_coord(bhi, G);
    return true;
}

// what star_pixel reports beside the sum (bhray_stars_resolve_host's statistics; the kernel passes nullptr)
struct StarPixelInfo {
    uint32_t state;            // 0 summed, 1 skipped by max_footprint, 2 skipped by BHRAY_STARS_MAX_CELLS
    uint32_t faces, cells, tested, accepted, reversed;
    float area;
};

// §23.2 - 6: the flux per steradian a pixel with four valid corners receives (before the gain).  Returns the number of stars accepted.
BH_HD uint32_t star_pixel(const StarSet& S, F3 d, F3 c00, F3 c10, F3 c01, F3 c11, F3& acc, StarPixelInfo* info) {
    acc = f3(0.0f, 0.0f, 0.0f);
    if (info) { info->state = 0; info->faces = info->cells = info->tested = info->accepted = info->reversed = 0; info->area = 0.0f; }
    // 2. the size test: four edges, two diagonals
    const F3 e0 = c10 - c00, e1 = c11 - c10, e2 = c01 - c11, e3 = c00 - c01, g0 = c11 - c00, g1 = c10 - c01;
    const float ch[6] = {dot(e0, e0), dot(e1, e1), dot(e2, e2), dot(e3, e3), dot(g0, g0), dot(g1, g1)};
    bool fits = true;
    for (int i = 0; i < 6; i++) if (!(ch[i] <= S.max_fp2)) fits = false;
    if (!fits) { if (info) info->state = 1; return 0; }
    // 3. the area
    const float A = 0.5f * length(cross(g0, g1));
    const float inv = 1.0f / max_(A, S.min_area);
    if (info) info->area = A;
    // 4. the boxes, counted first
    const uint32_t G = S.G;
    uint32_t total = 0, faces = 0;
    for (uint32_t f = 0; f < 6; f++) {
        uint32_t a0, a1, b0, b1;
        if (!star_face_box(f, c00, c10, c01, c11, G, a0, a1, b0, b1)) continue;
        total += (a1 - a0 + 1u) * (b1 - b0 + 1u);
        faces++;
    }
    if (info) { info->faces = faces; info->cells = total; }
    if (total > BHRAY_STARS_MAX_CELLS) { if (info) info->state = 2; return 0; }
    // 5. the edge functions' normals, one fixed winding: top, right, bottom, left
    const F3 nT = cross(c00, c10), nR = cross(c10, c11), nB = cross(c11, c01), nL = cross(c01, c00);
    uint32_t n = 0;
    for (uint32_t f = 0; f < 6; f++) {
        uint32_t a0, a1, b0, b1;
        if (!star_face_box(f, c00, c10, c01, c11, G, a0, a1, b0, b1)) continue;
        for (uint32_t bi = b0; bi <= b1; bi++) {
            const uint32_t row = (f * G + bi) * G;
            for (uint32_t ai = a0; ai <= a1; ai++) {
                const uint32_t k0 = S.prefix[row + ai], k1 = S.prefix[row + ai + 1u];
                for (uint32_t k = k0; k < k1; k++) {
                    const float4 sd = S.stars[2u * k];
                    const F3 s = f3(sd.x, sd.y, sd.z);
                    const float eT = dot(s, nT), eL = dot(s, nL), eB = dot(s, nB), eR = dot(s, nR);
                    const bool fwd = eT >= 0.0f && eL >= 0.0f && eB > 0.0f && eR > 0.0f;
                    const bool rev = eT <= 0.0f && eL <= 0.0f && eB < 0.0f && eR < 0.0f;
                    if (info) info->tested++;
                    if (!(fwd || rev) || !(dot(s, d) > 0.0f)) continue;
                    // 6. the sum
                    const float4 sf = S.stars[2u * k + 1u];
                    acc = acc + f3(sf.x, sf.y, sf.z) * inv;
                    n++;
                    if (info && !fwd) info->reversed++;
                }
            }
        }
    }
    if (info) info->accepted = n;
    return n;
}

// nullptr, or why bhray_set_stars refuses the arguments (include/bhray.h); params may be NULL (the defaults)
const char* stars_error(const bhray_star* stars, uint32_t n, const bhray_star_params* params);
// the index of n >= 1 checked stars: G, the stars sorted by (cell, original index) as two float4 each, the prefix array
void stars_build_index(const bhray_star* stars, uint32_t n, uint32_t& G, std::vector<float4>& sorted, std::vector<uint32_t>& prefix);
// the star pass over a whole frame_w x frame_h RGBA32F frame, added into the RGBA16F sky image in place.  Enqueues only.
hipError_t launch_stars(const StarSet& S, const float4* frame, uint2* sky_rgba16f, uint32_t frame_w, uint32_t frame_h, hipStream_t s);
// the host form over a frame (bhray_stars_resolve_host, bhray_diag_stars_pixel_info_host, bhray_accum_stars_resolve_host): add (w x h x 4 floats, may be NULL) and
// per-pixel information (bhray_diag.h's struct, may be NULL).  wrap_x: the frame is periodic in x - column -1 is column w - 1, column w is column 0.
int stars_resolve_host(const float* frame, uint32_t w, uint32_t h, bool wrap_x, const bhray_star* stars, uint32_t n, const bhray_star_params* params, float* add,
                       bhray_star_pixel_info* info);

}  // namespace bhray
