// forge3d_amd/csrc/f3d_umbra.h -- shadow-depth rasters on a live session (f3d_session_umbra): what one lane of k_umbra does.
// For every DEM sample: how far above the ground must a point over it stand to be lit from a direction -- the mounting height at
// which a panel, a mast or a crown catches the sun; the top of the terrain's shadow volume over the sample.  It is the sun mask
// (f3d_session_raster ALONG_DIRECTION) for every lift at once, as the clearance raster is the viewshed for every target height.
//
// THE CONTRACT.  Terrain only: a session with a mesh answers for its ground, as the horizon and clearance rasters do.  All
// arithmetic is f32, one rounding per written operation (f3d_math.h), so the host build (tests/umbra_host) and the device return
// the same bits.
// Sample n of the region is DEM sample (j, i); g = (x_i, h(i, j), z_j) is its lattice point: lattice_point (f3d_walk.h), lift 0.
// A direction is four f32 (dx, dy, dz, w), used as given, not normalised: toward the light, as an ALONG_DIRECTION target of
// f3d_session_raster.  w is reserved: 0.  With p(t) = (g.x + t dx, g.z + t dz), y(p) the bilinear surface of the cell under p
// and k = (dx^2 + dz^2) inv_two_r_prime under the curvature policy (CURVED on a scene whose curvature is enabled:
// horizon_curvature, make_ray's c2) and 0 otherwise, the ALONG_DIRECTION raster at lift L marches a ray whose height at
// parameter t is (h + L) + dy t + k t^2 (f3d_trace.h height_at: the curved march ADDS c2 t^2 to the ray, so relative to the ray
// the ground drops by k t^2 -- the sign of the k t^2 term of f3d_horizon.h), and the sample is lit exactly when that stays above
// y(p(t)) over the part of p(t) inside the footprint.  The smallest lift that is lit, and the raster's value, is
//     L* = max( +0, sup over t > 0 with p(t) inside the footprint of  y(p(t)) - k t^2 - dy t - h ).
// The footprint, the treatment of a zero component and "no cell beside the sample" are the walk's (f3d_walk.h).  No terrain
// along the direction (a border sample looking outward, a line along the far border edge): exactly +0.
// Special values, in this order:
//   qNaN   a non-finite component, or w != 0 (the device form; the host form refuses both);
//   qNaN   dx == dy == dz == 0;
//   dx == dz == 0 (straight up or down): +0 if dy > 0, +inf if dy < 0, with no walk;
//   qNaN   a walk that exceeds its step cap (walk_step_cap); no DEM reaches it.
// dy <= 0 is a legal direction with a horizontal part: the footprint is finite, so the supremum is.  (Dropping the sun below
// the horizontal is the Python wrapper's habit, as sun_hours'.)
//
// THE WALK is pyramid_walk (f3d_walk.h) as a ray from the sample, as the horizon's, with empty() = +0: the limit t -> 0+ of the
// functional is y(g) - h = 0, which is why the clamp of the contract costs nothing.
//
// THE LEAF.  With SampleRay's A, B, C of the cell (f3d_walk.h; C carrying hb - g.y: the cell's patch continued to the sample,
// minus h), the functional inside the cell is the quadratic q(t) = A t^2 + (B - dy) t + C over [t0, t1].  Its supremum is at t1, or --
// when A < 0 -- at the vertex t* = -(B - dy) / (2 A) if that lies strictly inside, where q(t*) = C + (B - dy) t* / 2.  The near
// end t0 is always answered already: by the previous cell, by a skipped node whose bound covers it, or by the initial 0.  There
// is no C / t: the horizon's quotient by a small parameter, and with it the amplification of C's rounding near the sample, is
// gone; the only division is the vertex's, taken in the cells that have one.
//
// THE NODE BOUND.  A node the line spends [t0, t1] in, whose band maximum is mx, holds y <= mx, so every point of it has
//     q(t) = y - h - k t^2 - dy t  <=  (mx - h) - k t0^2 - dy td,      td = t0 if dy >= 0 else t1
// (-k t^2 is largest at t0 since k >= 0; -dy t is largest at the near end for dy >= 0 and at the far end otherwise).  Each of the
// three terms is replaced by its own maximum over the node, taken where that term is largest -- the ends may differ, and the
// surface's maximum need not lie on the line at all --, which can only make the bound larger than the supremum, never smaller:
// a node is never skipped that could raise best.  The node is skipped when bound <= best, written !(bound <= best) so that a
// NaN descends.  best starts at +0 and only grows, so on open ground a lit sample's line falls below the band maxima after a
// cell or two, is skipped, climbs one level per skipped crossing and leaves the footprint in O(levels) steps; in shadow the
// cells up to the occluding crest raise best and are evaluated, the ground behind it is rejected at coarse levels.
//
// Measured against an independent float64 statement of the contract (tests/umbra_reference.py): tests/test_session_umbra_host.py.
#pragma once

#include "f3d_horizon.h"

namespace f3d {

// DEM sample (i, j) of sample n of the region, and its lattice point (lift 0)
F3D_HD V3 umbra_sample(const UmbraParams &R, uint32_t n, uint32_t &i, uint32_t &j) {
    return lattice_point(R.terrain, R.row0, R.col0, R.cols, n, 0.0f, i, j);
}

// The shadow depth's policy of pyramid_walk (f3d_walk.h): the header's node bound, and the header's leaf.
struct UmbraPolicy : SampleRay {
    float dy;
    bool rising;
    F3D_HD UmbraPolicy(const TerrainDev &T, float oy, uint32_t i, uint32_t j, float dx, float dy, float dz, float k)
        : SampleRay(T, oy, i, j, dx, dz, k), dy(dy), rising(dy >= 0.0f) {}
    static F3D_HD float empty() { return 0.0f; }
    F3D_HD bool may_raise(float mx, float t0, float t1, float best) const {
        return !(f_fma(-dy, rising ? t0 : t1, f_fma(-k * t0, t0, mx - oy)) <= best);
    }
    F3D_HD bool leaf(const TerrainDev &T, uint32_t nx, uint32_t nz, float t0, float t1, float, float &best) const {
        if (t1 > t0) {
            float A, B, C;
            quadratic(T, nx, nz, A, B, C);
            const float Bd = B - dy;
            best = f_max(best, f_fma(f_fma(A, t1, Bd), t1, C));
            if (A < 0.0f && Bd > 0.0f) {  // (a vertex at a positive parameter)
                const float ts = Bd / (-2.0f * A);
                if (ts > t0 && ts < t1) best = f_max(best, f_fma(0.5f * Bd, ts, C));
            }
        }
        return false;
    }
};

// One lane, one direction with a horizontal part: the supremum of the header for the sample (i, j) on g along (dx, dy, dz),
// clamped at +0.  Levels: see pyramid_walk.
template <class Levels>
F3D_HD float umbra_walk(const TerrainDev &T, V3 g, uint32_t i, uint32_t j, float dx, float dy, float dz, float k, uint32_t cap, const Levels &levels) {
    return pyramid_walk(T, g.x, g.z, dx, dz, i, j, cap, levels, UmbraPolicy(T, g.y, i, j, dx, dy, dz, k));
}

// One lane, one direction: the raster's value for the sample (i, j) whose lattice point is g.
template <class Levels>
F3D_HD float umbra_depth(const UmbraParams &R, V3 g, uint32_t i, uint32_t j, float4 d, const Levels &levels) {
    const float nan = f_from_bits(0x7FC00000u);
    if (!(f_finite(d.x) && f_finite(d.y) && f_finite(d.z) && d.w == 0.0f)) return nan;
    if (d.x == 0.0f && d.z == 0.0f) return d.y > 0.0f ? 0.0f : (d.y < 0.0f ? __builtin_inff() : nan);
    const float k = (R.curved != 0u && R.terrain.curvature_enabled != 0u) ? dot2(d.x, d.z, d.x, d.z) * R.terrain.inv_two_r_prime : 0.0f;
    return umbra_walk(R.terrain, g, i, j, d.x, d.y, d.z, k, R.step_cap, levels);
}

}  // namespace f3d
