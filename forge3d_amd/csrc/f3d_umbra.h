// forge3d_amd/csrc/f3d_umbra.h -- shadow-depth rasters on a live session (f3d_session_umbra): what one lane of k_umbra does.
// For every DEM sample: how far above the ground must a point over it stand to be lit from a direction -- the mounting height at
// which a panel, a mast or a crown catches the sun; the top of the terrain's shadow volume over the sample.  It is the sun mask
// (f3d_session_raster ALONG_DIRECTION) for every lift at once, as the clearance raster is the viewshed for every target height.
//
// THE CONTRACT.  Terrain only: a session with a mesh answers for its ground, as the horizon and clearance rasters do.  All
// arithmetic is f32, one rounding per written operation (f3d_math.h), so the host build (tests/umbra_host) and the device return
// the same bits.
// Sample n = r * cols + c of the region is DEM sample (j = row0 + r, i = col0 + c); its lattice point is clearance_sample's
// (f3d_clearance.h: raster_origin with lift 0),
//     g = (plane_at(origin_x, i, spacing_x), h(i, j), plane_at(origin_z, j, spacing_z)).
// A direction is four f32 (dx, dy, dz, w), used as given, not normalised: toward the light, as an ALONG_DIRECTION target of
// f3d_session_raster.  w is reserved: 0.  With p(t) = (g.x + t dx, g.z + t dz), y(p) the bilinear surface of the cell under p
// and k = (dx^2 + dz^2) inv_two_r_prime under the curvature policy (CURVED on a scene whose curvature is enabled:
// horizon_curvature, make_ray's c2) and 0 otherwise, the ALONG_DIRECTION raster at lift L marches a ray whose height at
// parameter t is (h + L) + dy t + k t^2 (f3d_trace.h height_at: the curved march ADDS c2 t^2 to the ray, so relative to the ray
// the ground drops by k t^2 -- the sign of the k t^2 term of f3d_horizon.h), and the sample is lit exactly when that stays above
// y(p(t)) over the part of p(t) inside the footprint.  The smallest lift that is lit, and the raster's value, is
//     L* = max( +0, sup over t > 0 with p(t) inside the footprint of  y(p(t)) - k t^2 - dy t - h ).
// The footprint, the treatment of a zero component and "no cell beside the sample" are horizon_walk's: cells
// [0, cell_w) x [0, cell_h), an axis with a zero component stepped as a forward one; a line that runs ALONG a lattice line
// (dx == 0 or dz == 0) lies in the cells on the higher-index side of it, so along the last lattice line of an axis -- the far
// border edge -- it meets no cell.  No terrain along the direction (a border sample looking outward, that far edge): exactly +0.
// Special values, in this order:
//   qNaN   a non-finite component, or w != 0 (the device form; the host form refuses both);
//   qNaN   dx == dy == dz == 0;
//   dx == dz == 0 (straight up or down): +0 if dy > 0, +inf if dy < 0, with no walk;
//   qNaN   a walk that exceeds its step cap (horizon_step_cap); no DEM reaches it.
// dy <= 0 is a legal direction with a horizontal part: the footprint is finite, so the supremum is.  (Dropping the sun below
// the horizontal is the Python wrapper's habit, as sun_hours'.)
//
// THE WALK is horizon_walk's stepping, unchanged: one current node (level, x, z), no stack; across the node's exit boundary to the
// neighbour of the same level, one level up when that crossing leaves the parent -- only out of a node that was skipped --, down
// into the child the line is in; the same plane parameters, the same integer offsets mu, mv of a cell's base corner from the
// sample.  It starts in the sample's own cell at level 0 with best = +0: the limit t -> 0+ of the functional is y(g) - h = 0,
// which is why the clamp of the contract costs nothing.  No tie bookkeeping, for horizon's reason: the functional is continuous
// across cell edges and corners.
//
// THE LEAF.  With horizon's A, B, C of the cell (C carrying hb - g.y: the cell's patch continued to the sample, minus h),
//     u = ux t - mu,  v = uz t - mv,   y = hb + e1 u + e2 v + tw u v
//     A = tw ux uz - k,   B = e1 ux + e2 uz - tw (mu uz + mv ux),   C = (hb - g.y) - e1 mu - e2 mv + tw mu mv
// the functional inside the cell is the quadratic q(t) = A t^2 + (B - dy) t + C over [t0, t1].  Its supremum is at t1, or --
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
// A hard step cap computed from the DEM (horizon_step_cap) ends a walk that has not left the footprint: qNaN.
//
// Measured against an independent float64 statement of the contract (tests/umbra_reference.py): tests/test_session_umbra_host.py.
#pragma once

#include "f3d_horizon.h"

namespace f3d {

// DEM sample (i, j) of sample n of the region, and its lattice point: clearance_sample's
F3D_HD V3 umbra_sample(const UmbraParams &R, uint32_t n, uint32_t &i, uint32_t &j) {
    const TerrainDev &T = R.terrain;
    const uint32_t r = n / R.cols, c = n - r * R.cols;
    j = R.row0 + r;
    i = R.col0 + c;
    const uint32_t cx = i < T.cell_w ? i : T.cell_w - 1u, cz = j < T.cell_h ? j : T.cell_h - 1u;
    const LeafRec rec = T.leaves[tiled_index(cx, cz, T.tiles_x[0])];
    const float h = pick4((i - cx) | ((j - cz) << 1), rec.h00, rec.h10, rec.h01, rec.h11);
    return V3{plane_at(T.origin_x, i, T.spacing_x), h + 0.0f, plane_at(T.origin_z, j, T.spacing_z)};
}

// One lane, one direction with a horizontal part: the supremum of the header for the sample (i, j) on g along (dx, dy, dz),
// clamped at +0.  Levels: band_entry(T, level, offset, shift), the per-level layout of T.bands (LDS on the device).
template <class Levels>
F3D_HD float umbra_walk(const TerrainDev &T, V3 g, uint32_t i, uint32_t j, float dx, float dy, float dz, float k, uint32_t cap, const Levels &levels) {
    const float inf = __builtin_inff();
    // an axis the line does not move along (flat): it runs along lattice line i for ever, in the column of that index (home)
    const bool x_flat = dx == 0.0f, z_flat = dz == 0.0f;
    const bool x_forward = !(dx < 0.0f), z_forward = !(dz < 0.0f);
    const uint32_t home_x = i, home_z = j;
    // the cell the line is in just after the sample; none: the sample looks out of the footprint (a flat axis counts as
    // forward, as in the march: along the LAST lattice line there is no cell -- the header's "footprint")
    if (x_forward ? i >= T.cell_w : i == 0u) return 0.0f;
    if (z_forward ? j >= T.cell_h : j == 0u) return 0.0f;
    uint32_t nx = x_forward ? i : i - 1u, nz = z_forward ? j : j - 1u;
    uint32_t level = 0u;
    const uint32_t top = T.mip_count - 1u;
    const float inv_x = safe_inv(dx), inv_z = safe_inv(dz);
    const float ux = f_abs(dx) * T.inv_spacing_x, uz = f_abs(dz) * T.inv_spacing_z;  // cells crossed per unit parameter
    const bool rising = dy >= 0.0f;
    float best = 0.0f, t_cur = 0.0f;
    for (uint32_t step = 0u; step < cap; step++) {
        // node extent in cells, clamped at ragged edges, and its plane parameters: the march's (f3d_march.h march_step)
        const uint32_t cx0 = nx << level, cz0 = nz << level;
        uint32_t cx1 = (nx + 1u) << level, cz1 = (nz + 1u) << level;
        cx1 = cx1 < T.cell_w ? cx1 : T.cell_w;
        cz1 = cz1 < T.cell_h ? cz1 : T.cell_h;
        const float tx0 = (plane_at(T.origin_x, cx0, T.spacing_x) - g.x) * inv_x;
        const float tx1 = (plane_at(T.origin_x, cx1, T.spacing_x) - g.x) * inv_x;
        const float tz0 = (plane_at(T.origin_z, cz0, T.spacing_z) - g.z) * inv_z;
        const float tz1 = (plane_at(T.origin_z, cz1, T.spacing_z) - g.z) * inv_z;
        const float x_in = x_flat ? -inf : f_min(tx0, tx1), x_out = x_flat ? inf : f_max(tx0, tx1);
        const float z_in = z_flat ? -inf : f_min(tz0, tz1), z_out = z_flat ? inf : f_max(tz0, tz1);
        const float t0 = f_max(f_max(x_in, z_in), 0.0f), t1 = f_min(x_out, z_out);
        uint32_t band_offset, band_shift;
        levels.band_entry(T, level, band_offset, band_shift);
        const float n = T.bands[band_offset + (nz << band_shift) + nx].mx - g.y;
        const float bound = f_fma(-dy, rising ? t0 : t1, f_fma(-k * t0, t0, n));
        const bool pass = !(t0 > t1) & !(bound <= best);
        if (pass && level > 0u) {
            // DOWN into the child the line is in at t_cur
            const uint32_t cl = level - 1u;
            const uint32_t xm = (2u * nx + 1u) << cl, zm = (2u * nz + 1u) << cl;
            const float txm = x_flat ? (xm <= home_x ? -inf : inf) : (plane_at(T.origin_x, xm, T.spacing_x) - g.x) * inv_x;
            const float tzm = z_flat ? (zm <= home_z ? -inf : inf) : (plane_at(T.origin_z, zm, T.spacing_z) - g.z) * inv_z;
            uint32_t ix = (x_forward != (txm <= t_cur)) ? 0u : 1u;
            uint32_t iz = (z_forward != (tzm <= t_cur)) ? 0u : 1u;
            if (!(xm < T.cell_w)) ix = 0u;  // the far half lies outside the cell grid
            if (!(zm < T.cell_h)) iz = 0u;
            nx = 2u * nx + ix;
            nz = 2u * nz + iz;
            level = cl;
        } else {
            if (pass && t1 > t0) {  // the leaf: the closed form of the header
                const LeafRec rec = T.leaves[tiled_index(nx, nz, T.tiles_x[0])];
                const uint32_t bx = x_forward ? nx : nx + 1u, bz = z_forward ? nz : nz + 1u;  // (a flat axis: nx = i, the base is the sample's own line)
                const uint32_t code = (bx - nx) | ((bz - nz) << 1);
                const float hb = pick4(code, rec.h00, rec.h10, rec.h01, rec.h11), hx = pick4(code ^ 1u, rec.h00, rec.h10, rec.h01, rec.h11);
                const float hz = pick4(code ^ 2u, rec.h00, rec.h10, rec.h01, rec.h11), hd = pick4(code ^ 3u, rec.h00, rec.h10, rec.h01, rec.h11);
                const float mu = x_flat ? 0.0f : (float)(x_forward ? bx - i : i - bx), mv = z_flat ? 0.0f : (float)(z_forward ? bz - j : j - bz);
                const float e1 = hx - hb, e2 = hz - hb, tw = (hd - hx) - e2;
                const float A = f_fma(tw * ux, uz, -k);
                const float Bd = f_fma(-tw, f_fma(mu, uz, mv * ux), f_fma(e1, ux, e2 * uz)) - dy;
                const float C = f_fma(tw * mu, mv, f_fma(-e2, mv, f_fma(-e1, mu, hb - g.y)));
                best = f_max(best, f_fma(f_fma(A, t1, Bd), t1, C));
                if (A < 0.0f && Bd > 0.0f) {  // (a vertex at a positive parameter)
                    const float ts = Bd / (-2.0f * A);
                    if (ts > t0 && ts < t1) best = f_max(best, f_fma(0.5f * Bd, ts, C));
                }
            }
            // ACROSS the exit boundary of this node (through a corner: both axes at once)
            const bool cross_x = x_out <= z_out, cross_z = z_out <= x_out;
            const uint32_t qx = nx + ((cross_x && x_forward) ? 1u : 0u) - ((cross_x && !x_forward) ? 1u : 0u);
            const uint32_t qz = nz + ((cross_z && z_forward) ? 1u : 0u) - ((cross_z && !z_forward) ? 1u : 0u);
            // (a backward step from column 0 wraps to 0xFFFFFFFF, whose shifted value is >= cell_w too)
            if (((qx << level) >= T.cell_w) | ((qz << level) >= T.cell_h)) return best;  // out of the footprint: done
            // (UP only from a node that was skipped, as horizon_walk)
            const bool up = !pass && level < top && (((qx ^ nx) | (qz ^ nz)) > 1u);
            nx = up ? qx >> 1 : qx;
            nz = up ? qz >> 1 : qz;
            level = up ? level + 1u : level;
            t_cur = f_max(t_cur, t1);
        }
    }
    return f_from_bits(0x7FC00000u);  // the cap: see the header
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
