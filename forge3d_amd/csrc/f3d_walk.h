// forge3d_amd/csrc/f3d_walk.h -- what the raster lanes share: the lattice point a DEM sample stands on (all five raster
// families), the samples a wave owns (region_sample) and the stackless walk over the min-max pyramid under the horizon,
// clearance and shadow-depth lanes (f3d_horizon.h, f3d_clearance.h, f3d_umbra.h: each a policy of pyramid_walk; horizon_lane
// and clearance_lane are the lane bodies the kernel and the host harness both call, with the Params by value, as the kernel
// holds them -- a reference costs scalar registers; k_umbra's loop stands in the kernel: profiles/README.md).
//
// All arithmetic is f32, one rounding per written operation (f3d_math.h), so the host builds (tests/*_host) and the device
// return the same bits.
//
// THE LATTICE is the one the march steps over: line X of the x axis is plane_at(origin_x, X, spacing_x), so a DEM sample lies
// EXACTLY on lines i and j, and the cell-local coordinate of a point is its parameter distance from the cell's planes times
// the cells the line crosses per unit parameter.
//
// THE FOOTPRINT is the one occluded() sees: cells [0, cell_w) x [0, cell_h), an axis with a zero component (a FLAT axis)
// stepped as a forward one.  A line that runs ALONG a lattice line (dx == 0 or dz == 0) stays on the sample's lattice line
// for ever and lies in the cells on the higher-index side of it -- the column of the sample's own index, `home` --, so along
// the last lattice line of an axis, the far border edge, it meets no cell, exactly as the march's root interval is empty
// there (tests/test_gpu_horizon.py brackets visibility() on those samples too).  Whether the line has a cell beside the
// SAMPLE is decided on the integers (i, j) and the signs of the direction before any parameter is computed; if it has none,
// the footprint being convex, it meets no terrain and the walk returns the policy's empty().
//
// NO TIE BOOKKEEPING.  The any-hit march has to visit the two cells a ray touches in one point when it passes exactly through
// a lattice corner (f3d_march.h "Corners"), because each cell's leaf test is a verdict of its own.  Here the quantity is a
// supremum of a CONTINUOUS function: the bilinear patches of neighbouring cells agree on their shared edge and corner, so a
// line that runs along a cell edge, or exactly through lattice corners, has one value whichever neighbouring cell is
// evaluated, and a cell touched in a single point adds a value the cells on either side already hold.  The walk therefore
// takes ONE cell per point of the line: along an edge the cell on the higher-index side, through a corner the diagonal
// neighbour.
//
// THE WALK is the march's stepping (f3d_march.h march_step: one current node (level, x, z), no stack; across the node's exit
// boundary to the neighbour of the same level, one level up when that crossing leaves the parent -- here only out of a node
// that was skipped --, down into the child the line is in) with another test: a node the line spends [t0, t1] in is entered
// only while the policy's bound over it, from the node's band maximum, can still raise `best` (may_raise; written so that a
// NaN descends), and a cell that is entered hands [t0, t1] to the policy's leaf.  best only grows, so what cannot matter is
// rejected at coarse levels.
// A hard step cap computed from the DEM (walk_step_cap) ends a walk that has not finished: the value is qNaN.  No DEM reaches
// it -- the line crosses at most cell_w + cell_h lattice lines and takes a bounded number of up / down steps per crossing --
// but nothing may spin.
//
// A POLICY supplies what differs between the families:
//   static constexpr bool kSegment   false: a ray from the sample, which is `home` itself: the walk starts in the sample's own
//                                    cell at level 0 with t_cur = 0 and ends where the line leaves the footprint.
//                                    true: the segment t in [0, 1] from a point off the lattice, possibly outside the
//                                    footprint, TO the sample (the line arrives at `home` along the direction, so the cell
//                                    beside the sample lies on the side the line comes from): the walk starts at the top
//                                    level with t_cur = t_start = max(t_in, 0) from the root's slab interval clipped to
//                                    [0, 1] (f3d_march.h march_root_interval's clipping; an empty interval: empty()), every
//                                    node's t1 is clipped at 1 and the walk is over when a node's exit is not below 1.  The
//                                    end point is the sample itself, on a lattice corner; the surface is continuous, so
//                                    whichever neighbouring cell the walk ends in serves.
//   static float empty()             the supremum over no terrain: the initial best, and the value of a line that meets no cell.
//   bool may_raise(mx, t0, t1, best) false: no point of a node with band maximum mx that the line spends [t0, t1] in can
//                                    raise best.
//   bool leaf(T, nx, nz, t0, t1, t_start, best)
//                                    cell (nx, nz) over [t0, t1] (t1 < t0 can occur: a touched corner): raise best.  The
//                                    near end t0 needs an answer only when !(t0 > t_start), in the first cell of the line
//                                    (t_start is 0 for a ray): every later t0 is a point the previous cell, or a skipped
//                                    node whose bound covers it, has already answered for.  true: the walk is over and
//                                    best is its value.
#pragma once

#include "f3d_trace.h"

namespace f3d {

// DEM sample (i, j) as the session holds it: a corner of the leaf table's record, exaggeration applied.  (The sample is corner
// (i - cx, j - cz) of cell (cx, cz); the last row and column have no cell of their own.)
F3D_HD float lattice_height(const TerrainDev &T, uint32_t i, uint32_t j) {
    const uint32_t cx = i < T.cell_w ? i : T.cell_w - 1u, cz = j < T.cell_h ? j : T.cell_h - 1u;
    const LeafRec rec = T.leaves[tiled_index(cx, cz, T.tiles_x[0])];
    return pick4((i - cx) | ((j - cz) << 1), rec.h00, rec.h10, rec.h01, rec.h11);
}

// DEM sample (j = row0 + r, i = col0 + c) of sample n = r * cols + c of a region, and its lifted lattice point
//     (plane_at(origin_x, i, spacing_x), h(i, j) + lift, plane_at(origin_z, j, spacing_z))
// -- plane_at is the march's own fma, so the point lies on the lattice the march steps over.  (lift 0.0f still writes h + lift:
// a -0 height becomes +0.)
F3D_HD V3 lattice_point(const TerrainDev &T, uint32_t row0, uint32_t col0, uint32_t cols, uint32_t n, float lift, uint32_t &i, uint32_t &j) {
    const uint32_t r = n / cols, c = n - r * cols;
    j = row0 + r;
    i = col0 + c;
    return V3{plane_at(T.origin_x, i, T.spacing_x), lattice_height(T, i, j) + lift, plane_at(T.origin_z, j, T.spacing_z)};
}

// A wave's samples (k_horizon, k_clearance, k_umbra: one wave a workgroup, one lane a sample): lane `lane` of wave `wave` ->
// sample n of a rows x cols region.  A wave owns 64 consecutive samples (the planes are written 256 contiguous bytes a wave),
// or with `block` an 8 x 8 block of the region (the 64 lines of an azimuth stay together at the coarse levels; measured:
// profiles/README.md).  false: the lane has no sample.  region_waves: the waves that cover the region, the launch's grid.
F3D_HD bool region_sample(uint32_t rows, uint32_t cols, uint32_t block, uint32_t wave, uint32_t lane, uint32_t &n) {
    n = wave * 64u + lane;
    bool have = n < rows * cols;
    if (block != 0u) {
        const uint32_t tiles_x = (cols + 7u) >> 3;
        const uint32_t r = (wave / tiles_x) * 8u + (lane >> 3), c = (wave % tiles_x) * 8u + (lane & 7u);
        have = r < rows && c < cols;
        n = r * cols + c;
    }
    return have;
}
F3D_HD uint32_t region_waves(uint32_t rows, uint32_t cols, uint32_t block) {
    return block != 0u ? ((cols + 7u) >> 3) * ((rows + 7u) >> 3) : (rows * cols + 63u) >> 6;
}

// the walk's step cap: every lattice line the line can cross, four times over, plus eight trips through the levels
F3D_HD uint32_t walk_step_cap(const TerrainDev &T) { return 4u * (T.cell_w + T.cell_h) + 8u * T.mip_count; }

// One lane, one line (ox + t dx, oz + t dz) with (dx, dz) finite and not both zero; home: the sample's (i, j).  Levels:
// band_entry(T, level, offset, shift), the per-level layout of T.bands (LDS on the device).
template <class Policy, class Levels>
F3D_HD float pyramid_walk(const TerrainDev &T, float ox, float oz, float dx, float dz, uint32_t home_x, uint32_t home_z, uint32_t cap,
                          const Levels &levels, const Policy &policy) {
    const float inf = __builtin_inff();
    const bool x_flat = dx == 0.0f, z_flat = dz == 0.0f;
    const bool x_forward = !(dx < 0.0f), z_forward = !(dz < 0.0f);
    if constexpr (Policy::kSegment) {
        // the cell beside the sample on the side the line comes from (a flat axis counts as forward)
        if (dx > 0.0f ? home_x == 0u : home_x >= T.cell_w) return Policy::empty();
        if (dz > 0.0f ? home_z == 0u : home_z >= T.cell_h) return Policy::empty();
    } else {
        // the cell the line is in just after the sample; none: the sample looks out of the footprint (a flat axis counts as
        // forward, as in the march: along the LAST lattice line there is no cell)
        if (x_forward ? home_x >= T.cell_w : home_x == 0u) return Policy::empty();
        if (z_forward ? home_z >= T.cell_h : home_z == 0u) return Policy::empty();
    }
    const uint32_t top = T.mip_count - 1u;
    const float inv_x = safe_inv(dx), inv_z = safe_inv(dz);
    uint32_t level, nx, nz;
    float t_start;
    if constexpr (Policy::kSegment) {
        // the root's slab interval, clipped to [0, 1]
        const float tx0 = (plane_at(T.origin_x, 0u, T.spacing_x) - ox) * inv_x, tx1 = (plane_at(T.origin_x, T.cell_w, T.spacing_x) - ox) * inv_x;
        const float tz0 = (plane_at(T.origin_z, 0u, T.spacing_z) - oz) * inv_z, tz1 = (plane_at(T.origin_z, T.cell_h, T.spacing_z) - oz) * inv_z;
        const float x_in = x_flat ? -inf : f_min(tx0, tx1), x_out = x_flat ? inf : f_max(tx0, tx1);
        const float z_in = z_flat ? -inf : f_min(tz0, tz1), z_out = z_flat ? inf : f_max(tz0, tz1);
        t_start = f_max(f_max(x_in, z_in), 0.0f);
        if (t_start > f_min(f_min(x_out, z_out), 1.0f)) return Policy::empty();
        level = top;
        nx = 0u;
        nz = 0u;
    } else {
        nx = x_forward ? home_x : home_x - 1u;
        nz = z_forward ? home_z : home_z - 1u;
        level = 0u;
        t_start = 0.0f;
    }
    float best = Policy::empty(), t_cur = t_start;
    for (uint32_t step = 0u; step < cap; step++) {
        // node extent in cells, clamped at ragged edges, and its plane parameters: the march's (f3d_march.h march_step)
        const uint32_t cx0 = nx << level, cz0 = nz << level;
        uint32_t cx1 = (nx + 1u) << level, cz1 = (nz + 1u) << level;
        cx1 = cx1 < T.cell_w ? cx1 : T.cell_w;
        cz1 = cz1 < T.cell_h ? cz1 : T.cell_h;
        const float tx0 = (plane_at(T.origin_x, cx0, T.spacing_x) - ox) * inv_x;
        const float tx1 = (plane_at(T.origin_x, cx1, T.spacing_x) - ox) * inv_x;
        const float tz0 = (plane_at(T.origin_z, cz0, T.spacing_z) - oz) * inv_z;
        const float tz1 = (plane_at(T.origin_z, cz1, T.spacing_z) - oz) * inv_z;
        const float x_in = x_flat ? -inf : f_min(tx0, tx1), x_out = x_flat ? inf : f_max(tx0, tx1);
        const float z_in = z_flat ? -inf : f_min(tz0, tz1), z_out = z_flat ? inf : f_max(tz0, tz1);
        const float exit = f_min(x_out, z_out);
        const float t0 = f_max(f_max(x_in, z_in), 0.0f);
        float t1 = exit;
        if constexpr (Policy::kSegment) t1 = f_min(exit, 1.0f);  // (the range ends at the sample)
        uint32_t band_offset, band_shift;
        levels.band_entry(T, level, band_offset, band_shift);
        const float mx = T.bands[band_offset + (nz << band_shift) + nx].mx;
        const bool pass = !(t0 > t1) & policy.may_raise(mx, t0, t1, best);
        if (pass && level > 0u) {
            // DOWN into the child the line is in at t_cur
            const uint32_t cl = level - 1u;
            const uint32_t xm = (2u * nx + 1u) << cl, zm = (2u * nz + 1u) << cl;
            const float txm = x_flat ? (xm <= home_x ? -inf : inf) : (plane_at(T.origin_x, xm, T.spacing_x) - ox) * inv_x;
            const float tzm = z_flat ? (zm <= home_z ? -inf : inf) : (plane_at(T.origin_z, zm, T.spacing_z) - oz) * inv_z;
            uint32_t ix = (x_forward != (txm <= t_cur)) ? 0u : 1u;
            uint32_t iz = (z_forward != (tzm <= t_cur)) ? 0u : 1u;
            if (!(xm < T.cell_w)) ix = 0u;  // the far half lies outside the cell grid
            if (!(zm < T.cell_h)) iz = 0u;
            nx = 2u * nx + ix;
            nz = 2u * nz + iz;
            level = cl;
        } else {
            if (pass && policy.leaf(T, nx, nz, t0, t1, t_start, best)) return best;
            if constexpr (Policy::kSegment)
                if (!(exit < 1.0f)) return best;  // the sample lies in (or on the border of) this node: done
            // ACROSS the exit boundary of this node (through a corner: both axes at once)
            const bool cross_x = x_out <= z_out, cross_z = z_out <= x_out;
            const uint32_t qx = nx + ((cross_x && x_forward) ? 1u : 0u) - ((cross_x && !x_forward) ? 1u : 0u);
            const uint32_t qz = nz + ((cross_z && z_forward) ? 1u : 0u) - ((cross_z && !z_forward) ? 1u : 0u);
            // (a backward step from column 0 wraps to 0xFFFFFFFF, whose shifted value is >= cell_w too)
            if (((qx << level) >= T.cell_w) | ((qz << level) >= T.cell_h)) return best;  // out of the footprint: done
            // (UP only from a node that was skipped: a line that has just raised best in a cell is on rising ground, where the
            // parent's neighbour would pass as well and hand the lane straight back down -- measured, profiles/README.md)
            const bool up = !pass && level < top && (((qx ^ nx) | (qz ^ nz)) > 1u);
            nx = up ? qx >> 1 : qx;
            nz = up ? qz >> 1 : qz;
            level = up ? level + 1u : level;
            t_cur = f_max(t_cur, t1);
        }
    }
    return f_from_bits(0x7FC00000u);  // the cap
}

// The node bound of a slope functional (y - oy - k t^2) / t, with n = mx - oy: every point of the node has
//     (y - oy - k t^2) / t  <=  n / t - k t  <=  n / ta - k t0,      ta = t0 if n > 0 else t1
// (n / t is largest at the near end for n > 0 and at the far end otherwise; -k t is largest at t0 since k >= 0: with k > 0 the
// two maxima are taken at different ends, which can only make the bound larger than the supremum, never smaller).  The node is
// skipped when bound <= best, tested without a division as  n - k t0 ta <= best ta  (ta >= 0; a NaN -- best = -inf with
// ta = 0 -- descends).
F3D_HD bool slope_may_raise(float n, float k, float t0, float t1, float best) {
    const float ta = n > 0.0f ? t0 : t1;
    return !(f_fma(-k * t0, ta, n) <= best * ta);
}

// What the policies of a ray from the sample (i, j) standing at height oy share.  Inside one cell the surface relative to
// the sample, y(p(t)) - oy - k t^2, is a quadratic A t^2 + B t + C.  The cell is taken from the corner the line enters it by
// (hb; hx, hz its neighbours along x and z, hd the opposite corner), which is mu >= 0 lattice lines ahead of the sample in x
// and mv in z -- integers, so in the sample's own cell mu = mv = 0 and C = hb - oy is -lift to the bit:
//     u = ux t - mu,  v = uz t - mv,   y = hb + e1 u + e2 v + tw u v,   e1 = hx - hb, e2 = hz - hb, tw = (hd - hx) - e2
//     A = tw ux uz - k,   B = e1 ux + e2 uz - tw (mu uz + mv ux),   C = (hb - oy) - e1 mu - e2 mv + tw mu mv
struct SampleRay {
    static constexpr bool kSegment = false;
    float oy, k, ux, uz;  // ux, uz: cells crossed per unit parameter
    uint32_t i, j;
    bool x_flat, z_flat, x_forward, z_forward;
    F3D_HD SampleRay(const TerrainDev &T, float oy, uint32_t i, uint32_t j, float dx, float dz, float k)
        : oy(oy), k(k), ux(f_abs(dx) * T.inv_spacing_x), uz(f_abs(dz) * T.inv_spacing_z), i(i), j(j), x_flat(dx == 0.0f), z_flat(dz == 0.0f),
          x_forward(!(dx < 0.0f)), z_forward(!(dz < 0.0f)) {}
    F3D_HD void quadratic(const TerrainDev &T, uint32_t nx, uint32_t nz, float &A, float &B, float &C) const {
        const LeafRec rec = T.leaves[tiled_index(nx, nz, T.tiles_x[0])];
        const uint32_t bx = x_forward ? nx : nx + 1u, bz = z_forward ? nz : nz + 1u;  // (a flat axis: nx = i, the base is the sample's own line)
        const uint32_t code = (bx - nx) | ((bz - nz) << 1);
        const float hb = pick4(code, rec.h00, rec.h10, rec.h01, rec.h11), hx = pick4(code ^ 1u, rec.h00, rec.h10, rec.h01, rec.h11);
        const float hz = pick4(code ^ 2u, rec.h00, rec.h10, rec.h01, rec.h11), hd = pick4(code ^ 3u, rec.h00, rec.h10, rec.h01, rec.h11);
        const float mu = x_flat ? 0.0f : (float)(x_forward ? bx - i : i - bx), mv = z_flat ? 0.0f : (float)(z_forward ? bz - j : j - bz);
        const float e1 = hx - hb, e2 = hz - hb, tw = (hd - hx) - e2;
        A = f_fma(tw * ux, uz, -k);
        B = f_fma(-tw, f_fma(mu, uz, mv * ux), f_fma(e1, ux, e2 * uz));
        C = f_fma(tw * mu, mv, f_fma(-e2, mv, f_fma(-e1, mu, hb - oy)));
    }
};

}  // namespace f3d
