// forge3d_amd/csrc/f3d_horizon.h -- horizon rasters on a live session (f3d_session_horizon): what one lane of k_horizon does.
//
// THE CONTRACT.  Terrain only: a session with a mesh answers for the ground.  Sample n = r * cols + c of the region is DEM
// sample (j = row0 + r, i = col0 + c) and stands on the lifted lattice point of the visibility rasters (f3d_raster.h
// raster_origin: the same corner of the leaf table's record, the same plane_at, the same lift; lift >= 0 here)
//     o = (plane_at(origin_x, i, spacing_x), h(i, j) + lift, plane_at(origin_z, j, spacing_z)).
// An azimuth is a horizontal direction (dx, dz), f32, used as given.  With p(t) = (o.x + t dx, o.z + t dz) and y(p) the
// bilinear surface of the cell under p (the leaf record's four corners), the horizon of the sample along the azimuth is
//     H = sup over t > 0 with p(t) inside the DEM's footprint of ( y(p(t)) - k t^2 - o.y ) / t
// where k = (dx^2 + dz^2) inv_two_r_prime under the curvature policy (CURVED on a scene whose curvature is enabled: make_ray's
// c2) and 0 otherwise -- the drop the curved march adds to a ray's height (f3d_trace.h height_at), so (dx, H, dz) is the
// grazing direction of occluded() for the same flag.  H is a rise per unit parameter: for a unit (dx, dz) the tangent of the
// horizon's elevation.  No terrain along the azimuth (a border sample looking outward): H = -inf.  With lift == 0 the
// supremum includes the limit t -> 0+, the surface's directional derivative.
// The footprint is the one occluded() sees: cells [0, cell_w) x [0, cell_h), an axis with a zero component stepped as a
// forward one.  A line that runs ALONG a lattice line (dx == 0 or dz == 0) lies in the cells on the higher-index side of it,
// so along the last lattice line of an axis -- the far border edge -- it meets no cell and H = -inf, exactly as the march's
// root interval is empty there (tests/test_gpu_horizon.py brackets visibility() on those samples too).
//
// The lattice is the one the march steps over: line X of the x axis is plane_at(origin_x, X, spacing_x), so the sample lies
// EXACTLY on lines i and j and the cell-local coordinate of a point is its parameter distance from the cell's planes
// times the cells the line crosses per unit parameter, (|dx| inv_spacing_x, |dz| inv_spacing_z).
//
// NO TIE BOOKKEEPING.  The any-hit march has to visit the two cells a ray touches in one point when it passes exactly through
// a lattice corner (f3d_march.h "Corners"), because each cell's leaf test is a verdict of its own.  Here the quantity is a
// supremum of a CONTINUOUS function: the bilinear patches of neighbouring cells agree on their shared edge and corner, so a
// line that runs along a cell edge, or exactly through lattice corners, has one value whichever neighbouring cell is
// evaluated, and a cell touched in a single point adds a value the cells on either side already hold.  The walk therefore
// takes ONE cell per point of the line: along an edge the cell on the higher-index side, through a corner the diagonal
// neighbour.
//
// THE LEAF.  Inside one cell the line spends [t0, t1] and y(p(t)) - o.y - k t^2 is a quadratic A t^2 + B t + C.  The cell is
// taken from the corner the line enters it by (hb; hx, hz its neighbours along x and z, hd the opposite corner), which is
// mu >= 0 lattice lines ahead of the sample in x and mv in z -- integers, so in the sample's own cell mu = mv = 0 and
// C = hb - o.y is -lift to the bit (0 with lift == 0: the limit t -> 0+ is B, with no 0 / 0):
//     u = ux t - mu,  v = uz t - mv,   y = hb + e1 u + e2 v + tw u v,   e1 = hx - hb, e2 = hz - hb, tw = (hd - hx) - e2
//     A = tw ux uz - k,   B = e1 ux + e2 uz - tw (mu uz + mv ux),   C = (hb - o.y) - e1 mu - e2 mv + tw mu mv
// The supremum of g(t) = A t + B + C / t over the segment is at t0, at t1, or at t* = sqrt(C / A) when t* lies strictly
// inside (a maximum exactly when A < 0 and C < 0; g(t*) = 2 A t* + B).  g(t0) is evaluated in the first cell only (t0 = 0):
// every later t0 is a point the previous cell, or a skipped node whose bound covers it, has already answered for.
//
// THE WALK is the march's stepping (f3d_march.h march_step: one current node (level, x, z), no stack; across the node's exit
// boundary to the neighbour of the same level, one level up when that crossing leaves the parent -- here only out of a node
// that was skipped --, down into the child the line is in) with another test.  A node the line spends [t0, t1] in, whose band
// maximum is mx, holds y <= mx, so with n = mx - o.y every point of it has
//     (y - o.y - k t^2) / t  <=  n / t - k t  <=  n / ta - k t0,      ta = t0 if n > 0 else t1
// (n / t is largest at the near end for n > 0 and at the far end otherwise; -k t is largest at t0 since k >= 0: with k > 0 the
// two maxima are taken at different ends, which can only make the bound larger than the supremum, never smaller).  The node is
// skipped when bound <= best, tested without a division as  n - k t0 ta <= best ta  (ta >= 0; a NaN -- best = -inf with
// ta = 0 -- descends).  best only grows, so terrain behind a crest and below the eye is rejected at coarse levels; on rising
// ground every cell up to the crest can raise the horizon and is evaluated (a band maximum cannot reject a node whose far end
// is much farther than its near end).
// A hard step cap computed from the DEM (horizon_step_cap) ends a walk that has not left the footprint: that azimuth of that
// sample is qNaN.  No DEM reaches it -- the line crosses at most cell_w + cell_h lattice lines and takes a bounded number of
// up / down steps per crossing -- but nothing may spin.
//
// All arithmetic is f32, one rounding per written operation (f3d_math.h), so the host build (tests/horizon_host) and the
// device return the same bits.  sky_view is the horizontal-surface sky-view factor of Dozier-Frew / Zaksek,
//     1 - (sum_k s_k) / K,   s_k = max(h, 0) / sqrt(1 + h^2),  h = H_k / sqrt(dx_k^2 + dz_k^2)
// (s_k: the sine of the horizon's elevation), summed for k = 0 .. K - 1 in f32 with every operation rounded on its own -- no
// fma, so that NumPy reproduces it from the planes bit for bit; -inf and NaN azimuths contribute 0.
#pragma once

#include "f3d_trace.h"

namespace f3d {

constexpr uint32_t kHorizonMaxAzimuths = 256u;

// the walk's step cap: every lattice line the line can cross, four times over, plus eight trips through the levels
F3D_HD uint32_t horizon_step_cap(const TerrainDev &T) { return 4u * (T.cell_w + T.cell_h) + 8u * T.mip_count; }

// DEM sample (i, j) of sample n of the region, and its lifted lattice point (f3d_raster.h raster_origin)
F3D_HD V3 horizon_origin(const HorizonParams &R, uint32_t n, uint32_t &i, uint32_t &j) {
    const TerrainDev &T = R.terrain;
    const uint32_t r = n / R.cols, c = n - r * R.cols;
    j = R.row0 + r;
    i = R.col0 + c;
    const uint32_t cx = i < T.cell_w ? i : T.cell_w - 1u, cz = j < T.cell_h ? j : T.cell_h - 1u;
    const LeafRec rec = T.leaves[tiled_index(cx, cz, T.tiles_x[0])];
    const float h = pick4((i - cx) | ((j - cz) << 1), rec.h00, rec.h10, rec.h01, rec.h11);
    return V3{plane_at(T.origin_x, i, T.spacing_x), h + R.lift, plane_at(T.origin_z, j, T.spacing_z)};
}

// The curvature coefficient of an azimuth: make_ray's c2.
F3D_HD float horizon_curvature(const HorizonParams &R, float dx, float dz) {
    const bool curved = R.curved != 0u && R.terrain.curvature_enabled != 0u;
    return curved ? dot2(dx, dz, dx, dz) * R.terrain.inv_two_r_prime : 0.0f;
}

// What the sample's sky-view sum takes from one azimuth (see the header: no fma).
F3D_HD float horizon_sky_term(float H, float dx, float dz) {
    const float h = H / f_sqrt(dx * dx + dz * dz);
    return h > 0.0f ? h / f_sqrt(1.0f + h * h) : 0.0f;  // (-inf, NaN: 0)
}

// One lane, one azimuth: the horizon of the sample (i, j) standing on o along (dx, dz).  Levels: band_entry(T, level, offset,
// shift), the per-level layout of T.bands (LDS on the device).
template <class Levels>
F3D_HD float horizon_walk(const TerrainDev &T, V3 o, uint32_t i, uint32_t j, float dx, float dz, float k, uint32_t cap, const Levels &levels) {
    const float inf = __builtin_inff();
    if (!(f_finite(dx) && f_finite(dz)) || (dx == 0.0f && dz == 0.0f)) return f_from_bits(0x7FC00000u);
    // an axis the line does not move along (flat): it runs along lattice line i for ever, in the column of that index (home)
    const bool x_flat = dx == 0.0f, z_flat = dz == 0.0f;
    const bool x_forward = !(dx < 0.0f), z_forward = !(dz < 0.0f);
    const uint32_t home_x = i, home_z = j;
    // the cell the line is in just after the sample; none: the sample looks out of the footprint (a flat axis counts as
    // forward, as in the march: along the LAST lattice line there is no cell -- the header's "footprint")
    if (x_forward ? i >= T.cell_w : i == 0u) return -inf;
    if (z_forward ? j >= T.cell_h : j == 0u) return -inf;
    uint32_t nx = x_forward ? i : i - 1u, nz = z_forward ? j : j - 1u;
    uint32_t level = 0u;
    const uint32_t top = T.mip_count - 1u;
    const float inv_x = safe_inv(dx), inv_z = safe_inv(dz);
    const float ux = f_abs(dx) * T.inv_spacing_x, uz = f_abs(dz) * T.inv_spacing_z;  // cells crossed per unit parameter
    float best = -inf, t_cur = 0.0f;
    for (uint32_t step = 0u; step < cap; step++) {
        // node extent in cells, clamped at ragged edges, and its plane parameters: the march's (f3d_march.h march_step)
        const uint32_t cx0 = nx << level, cz0 = nz << level;
        uint32_t cx1 = (nx + 1u) << level, cz1 = (nz + 1u) << level;
        cx1 = cx1 < T.cell_w ? cx1 : T.cell_w;
        cz1 = cz1 < T.cell_h ? cz1 : T.cell_h;
        const float tx0 = (plane_at(T.origin_x, cx0, T.spacing_x) - o.x) * inv_x;
        const float tx1 = (plane_at(T.origin_x, cx1, T.spacing_x) - o.x) * inv_x;
        const float tz0 = (plane_at(T.origin_z, cz0, T.spacing_z) - o.z) * inv_z;
        const float tz1 = (plane_at(T.origin_z, cz1, T.spacing_z) - o.z) * inv_z;
        const float x_in = x_flat ? -inf : f_min(tx0, tx1), x_out = x_flat ? inf : f_max(tx0, tx1);
        const float z_in = z_flat ? -inf : f_min(tz0, tz1), z_out = z_flat ? inf : f_max(tz0, tz1);
        const float t0 = f_max(f_max(x_in, z_in), 0.0f), t1 = f_min(x_out, z_out);
        uint32_t band_offset, band_shift;
        levels.band_entry(T, level, band_offset, band_shift);
        const float n = T.bands[band_offset + (nz << band_shift) + nx].mx - o.y;
        const float ta = n > 0.0f ? t0 : t1;
        const bool pass = !(t0 > t1) & !(f_fma(-k * t0, ta, n) <= best * ta);
        if (pass && level > 0u) {
            // DOWN into the child the line is in at t_cur
            const uint32_t cl = level - 1u;
            const uint32_t xm = (2u * nx + 1u) << cl, zm = (2u * nz + 1u) << cl;
            const float txm = x_flat ? (xm <= home_x ? -inf : inf) : (plane_at(T.origin_x, xm, T.spacing_x) - o.x) * inv_x;
            const float tzm = z_flat ? (zm <= home_z ? -inf : inf) : (plane_at(T.origin_z, zm, T.spacing_z) - o.z) * inv_z;
            uint32_t ix = (x_forward != (txm <= t_cur)) ? 0u : 1u;
            uint32_t iz = (z_forward != (tzm <= t_cur)) ? 0u : 1u;
            if (!(xm < T.cell_w)) ix = 0u;  // the far half lies outside the cell grid
            if (!(zm < T.cell_h)) iz = 0u;
            nx = 2u * nx + ix;
            nz = 2u * nz + iz;
            level = cl;
        } else {
            if (pass) {  // the leaf: the closed form of the header
                const LeafRec rec = T.leaves[tiled_index(nx, nz, T.tiles_x[0])];
                const uint32_t bx = x_forward ? nx : nx + 1u, bz = z_forward ? nz : nz + 1u;  // (a flat axis: nx = i, the base is the sample's own line)
                const uint32_t code = (bx - nx) | ((bz - nz) << 1);
                const float hb = pick4(code, rec.h00, rec.h10, rec.h01, rec.h11), hx = pick4(code ^ 1u, rec.h00, rec.h10, rec.h01, rec.h11);
                const float hz = pick4(code ^ 2u, rec.h00, rec.h10, rec.h01, rec.h11), hd = pick4(code ^ 3u, rec.h00, rec.h10, rec.h01, rec.h11);
                const float mu = x_flat ? 0.0f : (float)(x_forward ? bx - i : i - bx), mv = z_flat ? 0.0f : (float)(z_forward ? bz - j : j - bz);
                const float e1 = hx - hb, e2 = hz - hb, tw = (hd - hx) - e2;
                const float A = f_fma(tw * ux, uz, -k);
                const float B = f_fma(-tw, f_fma(mu, uz, mv * ux), f_fma(e1, ux, e2 * uz));
                const float C = f_fma(tw * mu, mv, f_fma(-e2, mv, f_fma(-e1, mu, hb - o.y)));
                if (!(t0 > 0.0f)) best = f_max(best, C < 0.0f ? -inf : B);  // the sample's own cell: the limit t -> 0+
                if (t1 > t0) {
                    best = f_max(best, f_fma(A, t1, B) + C / t1);
                    if (A < 0.0f && C < 0.0f) {
                        const float ts = f_sqrt(C / A);
                        if (ts > t0 && ts < t1) best = f_max(best, f_fma(2.0f * A, ts, B));
                    }
                }
            }
            // ACROSS the exit boundary of this node (through a corner: both axes at once)
            const bool cross_x = x_out <= z_out, cross_z = z_out <= x_out;
            const uint32_t qx = nx + ((cross_x && x_forward) ? 1u : 0u) - ((cross_x && !x_forward) ? 1u : 0u);
            const uint32_t qz = nz + ((cross_z && z_forward) ? 1u : 0u) - ((cross_z && !z_forward) ? 1u : 0u);
            // (a backward step from column 0 wraps to 0xFFFFFFFF, whose shifted value is >= cell_w too)
            if (((qx << level) >= T.cell_w) | ((qz << level) >= T.cell_h)) return best;  // out of the footprint: done
            // (UP only from a node that was skipped: a line that has just raised the horizon in a cell is on rising ground, where the
            // parent's neighbour would pass as well and hand the lane straight back down -- measured, profiles/README.md)
            const bool up = !pass && level < top && (((qx ^ nx) | (qz ^ nz)) > 1u);
            nx = up ? qx >> 1 : qx;
            nz = up ? qz >> 1 : qz;
            level = up ? level + 1u : level;
            t_cur = f_max(t_cur, t1);
        }
    }
    return f_from_bits(0x7FC00000u);  // the cap: see the header
}

}  // namespace f3d
