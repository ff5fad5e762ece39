// forge3d_amd/csrc/f3d_clearance.h -- clearance rasters on a live session (f3d_session_clearance): what one lane of
// k_clearance does.  For every DEM sample: how far above the ground must a target stand for an observer to see it -- the
// "above ground level" output of a GIS viewshed tool, i.e. the viewshed for every target height at once.
//
// THE CONTRACT.  Terrain only: a session with a mesh answers for the ground, as the horizon raster does.  All arithmetic is
// f32, one rounding per written operation (f3d_math.h), so the host build (tests/clearance_host) and the device return the
// same bits.
// Sample n = r * cols + c of the region is DEM sample (j = row0 + r, i = col0 + c); its lattice point is raster_origin's
// (f3d_raster.h) with lift 0,
//     g = (plane_at(origin_x, i, spacing_x), h(i, j), plane_at(origin_z, j, spacing_z)).
// An observer is four f32 (x, Y, z, w), as a TOWARD_POINT target of f3d_session_raster; w > 0 is a maximum horizontal
// distance.  With dx = x - g.x, dz = z - g.z, hd2 = dx dx + dz dz and k = hd2 inv_two_r_prime under the curvature policy
// (CURVED on a scene whose curvature is enabled; else 0), raster_visible at lift L marches a ray whose height at parameter
// t in (0, 1) is (h + L)(1 - t) + t Y - k t (1 - t), and the sample is seen exactly when that stays above the bilinear
// surface y(p(t)), p(t) = (g.x + t dx, g.z + t dz), over the part of p(t) inside the footprint.  The smallest lift seen is
//     L* = sup over t in (0, 1), p(t) in the footprint, of  (y(p(t)) - t Y) / (1 - t) + k t - h.
// Written from the observer's end (s = 1 - t, origin P = (x, z), direction e = (-dx, -dz)):
//     L* = (Y + k - h) + H,     H = sup over s in (0, 1) of ( y(P + s e) - k s^2 - Y ) / s
// -- H is the horizon of f3d_horizon.h from an arbitrary point, its range cut at s = 1.  The raster's value is max(L*, +0):
// in real arithmetic the limit s -> 1 makes L* >= 0, the clamp removes the rounding below it.
// Special values, in this order:
//   qNaN   a non-finite observer component (the device form; the host form refuses it), or an hd2 that overflows;
//   +inf   hd2 > w w: never seen within range;
//   hd2 == 0 (the sample straight under or over the observer): +inf if Y < h, else 0, with no walk;
//   0      no terrain between (H = -inf): the line has no cell beside the sample (below), or misses the footprint;
//   +inf   the observer lies under the surface (P in the footprint and y(P) > Y): the walk's first leaf gives it, C > 0 as
//          s -> 0+.
// The footprint is the march's, as the horizon raster states it: cells [0, cell_w) x [0, cell_h), an axis with a zero
// component stepped as a forward one -- the line then runs along lattice line i (x == g.x exactly) in the cells on the
// higher-index side, and along the DEM's last lattice line it meets no cell.  Whether the line has a cell beside the SAMPLE
// is decided on the integers (i, j) and the signs of (dx, dz) before any parameter is computed: if it has none, the
// footprint being convex, there is no terrain between and the value is exactly 0.
// A walk that exceeds its step cap (clearance_step_cap) writes qNaN; no DEM reaches the cap.
//
// THE WALK is horizon_walk's stepping (one current node, no stack; across the node's exit boundary, up only out of a node that
// was skipped, down into the child the line is in; the same plane parameters; the same node bound n - k t0 ta <= best ta
// with n = mx - Y) from the OBSERVER, because best rises early there -- near terrain sets the horizon -- and far subtrees are
// then rejected at coarse levels; walked from the sample the decisive blockers would come last and nothing would prune.
// It differs from horizon_walk in three ways:
//   * the origin is off the lattice and possibly outside the footprint: the walk starts at the top level with
//     t_cur = t_start = max(t_in, 0) from the root's slab interval (f3d_march.h march_root_interval's clipping);
//   * the range ends at s = 1: every node's t1 is clipped there and the walk is over when a node's exit is not below 1.  The
//     end point is the sample itself, on a lattice corner; the surface is continuous, so whichever neighbouring cell the
//     walk ends in serves;
//   * the leaf's cell-local coordinates have no integer offsets.  They are taken from the cell's OWN (0, 0) corner,
//         u = au + bu s,  au = (x - X0) inv_spacing_x,  bu = e.x inv_spacing_x      (v likewise along z)
//     which cancels least where it matters: C below is the cell's patch continued to the observer minus Y, and it is
//     divided by s -- a cell near the observer (small s, the quotient amplified) has a small au that the subtraction gives
//     almost exactly, a far cell's large au meets a large s.  (Counting lattice lines from the sample keeps the offsets
//     integers but continues every patch over the whole sight line first and then divides the near ones by a small s.)
//         y = h00 + e1 u + e2 v + tw u v,   e1 = h10 - h00, e2 = h01 - h00, tw = (h11 - h10) - e2
//         A = tw bu bv - k,   B = e1 bu + e2 bv + tw (au bv + av bu),   C = (h00 - Y) + e1 au + e2 av + tw au av
//     and the supremum of g(s) = A s + B + C / s over the cell's [t0, t1] is at t0, at t1, or at s* = sqrt(C / A) strictly
//     inside (A < 0 and C < 0).  g(t0) is evaluated only where nothing before has answered for it: in the first cell of the
//     line, t0 = t_start -- the limit s -> 0+ when the observer is inside the footprint (C > 0: +inf; C == 0: B), the
//     footprint's border otherwise.
// Measured against a float64 statement of the first form (tests/clearance_reference.py): tests/test_session_clearance_host.py.
#pragma once

#include "f3d_trace.h"

namespace f3d {

// the walk's step cap: every lattice line the line can cross, four times over, plus eight trips through the levels
F3D_HD uint32_t clearance_step_cap(const TerrainDev &T) { return 4u * (T.cell_w + T.cell_h) + 8u * T.mip_count; }

// DEM sample (i, j) of sample n of the region, and its lattice point (f3d_raster.h raster_origin with lift 0)
F3D_HD V3 clearance_sample(const ClearanceParams &R, uint32_t n, uint32_t &i, uint32_t &j) {
    const TerrainDev &T = R.terrain;
    const uint32_t r = n / R.cols, c = n - r * R.cols;
    j = R.row0 + r;
    i = R.col0 + c;
    const uint32_t cx = i < T.cell_w ? i : T.cell_w - 1u, cz = j < T.cell_h ? j : T.cell_h - 1u;
    const LeafRec rec = T.leaves[tiled_index(cx, cz, T.tiles_x[0])];
    const float h = pick4((i - cx) | ((j - cz) << 1), rec.h00, rec.h10, rec.h01, rec.h11);
    return V3{plane_at(T.origin_x, i, T.spacing_x), h + 0.0f, plane_at(T.origin_z, j, T.spacing_z)};
}

// One lane, one observer: H of the header for the sample (i, j), walked from P = (x, Y, z) along e = (ex, ez) over s in (0, 1).
// Levels: band_entry(T, level, offset, shift), the per-level layout of T.bands (LDS on the device).
template <class Levels>
F3D_HD float clearance_walk(const TerrainDev &T, V3 P, float ex, float ez, uint32_t i, uint32_t j, float k, uint32_t cap, const Levels &levels) {
    const float inf = __builtin_inff();
    // an axis the line does not move along (flat): it runs along the sample's lattice line, in the column of that index (home)
    const bool x_flat = ex == 0.0f, z_flat = ez == 0.0f;
    const bool x_forward = !(ex < 0.0f), z_forward = !(ez < 0.0f);
    const uint32_t home_x = i, home_z = j;
    // the cell beside the sample on the observer's side (the line arrives along e, so it lies on the side of -e; a flat axis
    // counts as forward): none, and there is no terrain between -- the header's "footprint"
    if (ex > 0.0f ? i == 0u : i >= T.cell_w) return -inf;
    if (ez > 0.0f ? j == 0u : j >= T.cell_h) return -inf;
    const float inv_x = safe_inv(ex), inv_z = safe_inv(ez);
    const float bu = ex * T.inv_spacing_x, bv = ez * T.inv_spacing_z;  // cells per unit parameter, signed
    const uint32_t top = T.mip_count - 1u;
    // the root's slab interval, clipped to [0, 1]
    float t_start;
    {
        const float tx0 = (plane_at(T.origin_x, 0u, T.spacing_x) - P.x) * inv_x, tx1 = (plane_at(T.origin_x, T.cell_w, T.spacing_x) - P.x) * inv_x;
        const float tz0 = (plane_at(T.origin_z, 0u, T.spacing_z) - P.z) * inv_z, tz1 = (plane_at(T.origin_z, T.cell_h, T.spacing_z) - P.z) * inv_z;
        const float x_in = x_flat ? -inf : f_min(tx0, tx1), x_out = x_flat ? inf : f_max(tx0, tx1);
        const float z_in = z_flat ? -inf : f_min(tz0, tz1), z_out = z_flat ? inf : f_max(tz0, tz1);
        t_start = f_max(f_max(x_in, z_in), 0.0f);
        if (t_start > f_min(f_min(x_out, z_out), 1.0f)) return -inf;
    }
    uint32_t level = top, nx = 0u, nz = 0u;
    float best = -inf, t_cur = t_start;
    for (uint32_t step = 0u; step < cap; step++) {
        // node extent in cells, clamped at ragged edges, and its plane parameters: the march's (f3d_march.h march_step)
        const uint32_t cx0 = nx << level, cz0 = nz << level;
        uint32_t cx1 = (nx + 1u) << level, cz1 = (nz + 1u) << level;
        cx1 = cx1 < T.cell_w ? cx1 : T.cell_w;
        cz1 = cz1 < T.cell_h ? cz1 : T.cell_h;
        const float tx0 = (plane_at(T.origin_x, cx0, T.spacing_x) - P.x) * inv_x;
        const float tx1 = (plane_at(T.origin_x, cx1, T.spacing_x) - P.x) * inv_x;
        const float tz0 = (plane_at(T.origin_z, cz0, T.spacing_z) - P.z) * inv_z;
        const float tz1 = (plane_at(T.origin_z, cz1, T.spacing_z) - P.z) * inv_z;
        const float x_in = x_flat ? -inf : f_min(tx0, tx1), x_out = x_flat ? inf : f_max(tx0, tx1);
        const float z_in = z_flat ? -inf : f_min(tz0, tz1), z_out = z_flat ? inf : f_max(tz0, tz1);
        const float exit = f_min(x_out, z_out);
        const float t0 = f_max(f_max(x_in, z_in), 0.0f), t1 = f_min(exit, 1.0f);  // (the range ends at the sample)
        uint32_t band_offset, band_shift;
        levels.band_entry(T, level, band_offset, band_shift);
        const float n = T.bands[band_offset + (nz << band_shift) + nx].mx - P.y;
        const float ta = n > 0.0f ? t0 : t1;
        const bool pass = !(t0 > t1) & !(f_fma(-k * t0, ta, n) <= best * ta);
        if (pass && level > 0u) {
            // DOWN into the child the line is in at t_cur
            const uint32_t cl = level - 1u;
            const uint32_t xm = (2u * nx + 1u) << cl, zm = (2u * nz + 1u) << cl;
            const float txm = x_flat ? (xm <= home_x ? -inf : inf) : (plane_at(T.origin_x, xm, T.spacing_x) - P.x) * inv_x;
            const float tzm = z_flat ? (zm <= home_z ? -inf : inf) : (plane_at(T.origin_z, zm, T.spacing_z) - P.z) * inv_z;
            uint32_t ix = (x_forward != (txm <= t_cur)) ? 0u : 1u;
            uint32_t iz = (z_forward != (tzm <= t_cur)) ? 0u : 1u;
            if (!(xm < T.cell_w)) ix = 0u;  // the far half lies outside the cell grid
            if (!(zm < T.cell_h)) iz = 0u;
            nx = 2u * nx + ix;
            nz = 2u * nz + iz;
            level = cl;
        } else {
            if (pass) {  // the leaf: the closed form of the header, from the cell's own (0, 0) corner
                const LeafRec rec = T.leaves[tiled_index(nx, nz, T.tiles_x[0])];
                const float au = (P.x - plane_at(T.origin_x, nx, T.spacing_x)) * T.inv_spacing_x;
                const float av = (P.z - plane_at(T.origin_z, nz, T.spacing_z)) * T.inv_spacing_z;
                const float e1 = rec.h10 - rec.h00, e2 = rec.h01 - rec.h00, tw = (rec.h11 - rec.h10) - e2;
                const float A = f_fma(tw * bu, bv, -k);
                const float B = f_fma(tw, f_fma(au, bv, av * bu), f_fma(e1, bu, e2 * bv));
                const float C = f_fma(tw * au, av, f_fma(e2, av, f_fma(e1, au, rec.h00 - P.y)));
                if (!(t0 > t_start)) {  // the first cell of the line: nothing before it has answered for its near end
                    if (t0 > 0.0f) {
                        best = f_max(best, f_fma(A, t0, B) + C / t0);
                    } else {
                        if (C > 0.0f) return inf;  // the observer lies under the surface
                        if (!(C < 0.0f)) best = f_max(best, B);  // ... exactly on it: the limit s -> 0+
                    }
                }
                if (t1 > t0) {
                    best = f_max(best, f_fma(A, t1, B) + C / t1);
                    if (A < 0.0f && C < 0.0f) {
                        const float ts = f_sqrt(C / A);
                        if (ts > t0 && ts < t1) best = f_max(best, f_fma(2.0f * A, ts, B));
                    }
                }
            }
            if (!(exit < 1.0f)) return best;  // the sample lies in (or on the border of) this node: done
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

// One lane, one observer: the raster's value for the sample (i, j) whose lattice point is g.
template <class Levels>
F3D_HD float clearance_height(const ClearanceParams &R, V3 g, uint32_t i, uint32_t j, float4 ob, const Levels &levels) {
    const float inf = __builtin_inff(), nan = f_from_bits(0x7FC00000u);
    if (!(f_finite(ob.x) && f_finite(ob.y) && f_finite(ob.z) && f_finite(ob.w))) return nan;
    const float dx = ob.x - g.x, dz = ob.z - g.z;
    const float hd2 = dx * dx + dz * dz;
    if (!f_finite(hd2)) return nan;
    if (ob.w > 0.0f && hd2 > ob.w * ob.w) return inf;
    if (hd2 == 0.0f) return ob.y < g.y ? inf : 0.0f;
    const float k = (R.curved != 0u && R.terrain.curvature_enabled != 0u) ? hd2 * R.terrain.inv_two_r_prime : 0.0f;
    const float H = clearance_walk(R.terrain, V3{ob.x, ob.y, ob.z}, -dx, -dz, i, j, k, R.step_cap, levels);
    if (H != H) return nan;
    const float L = ((ob.y + k) - g.y) + H;
    return L > 0.0f ? L : 0.0f;
}

}  // namespace f3d
