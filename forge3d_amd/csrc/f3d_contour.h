// forge3d_amd/csrc/f3d_contour.h -- contour lines of a live session's terrain (f3d_session_contours, f3d_session_paint_contours):
// what one lane of k_contour_count / k_contour_emit does for its cell.  Host and device: tests/contour_host runs the same bodies
// on the CPU over whole 64-lane waves, and the device returns those bits, in that order.
//
// THE CONTRACT.  All arithmetic is f32, one rounding per written operation (the library and the host harness are compiled with
// -ffp-contract=off; the only fused multiply-add is plane_at's own, the lattice's); division is the correctly rounded form.
//
// Inputs.  Heights are the leaf table's: f32(h * exaggeration), the y that ground() and pick() return, four corners a cell
// (h00 at sample (i, j), h10 at (i + 1, j), h01 at (i, j + 1), h11 at (i + 1, j + 1)).  Levels are in the same unit, finite and
// strictly ascending, at most kContourMaxLevels of them.  The region is a region of CELLS (row0, col0, rows, cols) inside the
// cell_h x cell_w grid.
//
// Case and table (marching squares).  Per cell and level the case is the sum of the corners' bits, a corner's bit set when
// h >= level: h00 -> 1, h10 -> 2, h01 -> 4, h11 -> 8.  The cell's four lattice edges are B (h00-h10, row j), R (h10-h11, column
// i + 1), T (h01-h11, row j + 1) and L (h00-h01, column i); a case's segments, each from its first crossing to its second:
//      1 L-B    2 B-R    3 L-R    4 T-L    5 T-B    6 B-R, T-L    7 T-R
//      8 R-T    9 L-B, R-T    10 B-T    11 L-T    12 R-L    13 R-B    14 B-L          0 and 15: nothing
// The two saddles (6, 9) are always paired as written: no decider from the bilinear patch.  Every edge a case names is crossed:
// one of its samples has h >= level, the other h < level.
//
// A CROSSING BELONGS TO ITS LATTICE EDGE, NOT TO A CELL.  On the x-edge from sample (i, j) to (i + 1, j), a = the sample of lower
// index:
//      t = (level - h_a) / (h_b - h_a)          x = plane_at(origin_x, i, spacing_x) + t * spacing_x          z = plane_at(origin_z, j, spacing_z)
// and the z-edge likewise with x and z exchanged.  When t == 0 or t == 1 the crossing takes that sample's own plane_at value.
// Therefore the two cells that share an edge compute the same bits; all crossings that fall on one sample coincide bit for
// bit; and 0 <= t <= 1 always: on a crossed edge h_a < level <= h_b or h_b < level <= h_a, numerator and denominator have one
// sign with |level - h_a| <= |h_b - h_a|, and both roundings (of the differences, of the quotient) are monotone.
// (The rule this restates guards its quotient with "|h2 - h1| < 1e-6 -> t = 0.5".  A crossed edge has h_a != h_b, so in f32 that
// branch can only change an edge whose samples differ by less than 1e-6 -- and it exists to keep a quotient finite on edges that
// are NOT crossed, which that rule evaluates and then does not use.  Here only crossed edges are evaluated, where the quotient
// is in [0, 1] by the argument above: the branch has no counterpart.)
// A level that passes exactly through a sample gives segments of length zero; they are emitted, as that rule emits them.
//
// ORDER OF THE OUTPUT ("block order").  Blocks of 8 x 8 cells aligned to the DEM's cell grid (not to the region), row-major over
// blocks; cells row-major inside a block; levels ascending inside a cell; a case's segments in table order.  It depends on
// nothing else: not on the launch shape, not on the region's alignment, not on the cull.
//
// Output record: float[4] = (ax, az, bx, bz) in world x-z, and a parallel uint32 index into `levels`; or a PaintPrim
// (f3d_paint.h) with v = (a, b, b), the call's colour on all three vertices, feature 0, reserved 0 -- the bits f3d_session_paint
// builds on the host for a `lines` call without feature ids.
//
// THE CULL.  A cell emits for a level iff  min(corners) < level <= max(corners).  The wave reads its block's record of level 3
// of `bands` (8 x 8 cells; a pyramid without a level 3 -- fewer than five cells a side -- has a root that covers the whole grid)
// and bisects the sorted levels to [first level > mn, first level > mx); each lane bisects inside that range to its own cell's.
// A band's (mn, mx) are exact minima and maxima of the cells' corners, so the cull drops nothing.
//
// Two passes over the same lane body (contour_lane_range, then contour_lane_count or contour_lane_emit): per block a total, an
// exclusive scan of the totals, then every lane writes at the block's offset plus the wave-exclusive prefix of its count.
#pragma once

#include "f3d_paint.h"
#include "f3d_trace.h"

namespace f3d {

constexpr uint32_t kContourMaxLevels = 65536u;
constexpr uint32_t kContourB = 0u, kContourR = 1u, kContourT = 2u, kContourL = 3u;
// the table above, a nibble a case: first crossing | second crossing << 2 of the first segment; the saddles' second segments
constexpr uint64_t kContourFirst = 0x0C1DB839642E7430ull;
constexpr uint32_t kContourSecond6 = kContourT | kContourL << 2, kContourSecond9 = kContourR | kContourT << 2;

struct ContourParams {
    TerrainDev terrain;
    uint32_t row0, col0, rows, cols;   // the region, in cells
    uint32_t bx0, bz0, nbx, nbz;       // the blocks it touches: contour_blocks()
    const float *levels;
    uint32_t level_count;
    uint32_t cull;                     // 0: every block walks every level (A/B, same results)
    uint64_t *totals;                  // nbx * nbz + 1 words: segments a block, then 0
    const uint64_t *offsets;           // their exclusive scan: offsets[nbx * nbz] is the total
    uint64_t capacity;                 // records the outputs hold
    float *segments;                   // capacity x 4, or null
    uint32_t *level_index;             // capacity, or null
    PaintPrim *prims;                  // capacity records, or null (then segments / level_index)
    float rgba[4];
};

F3D_HD void contour_blocks(ContourParams &P) {
    P.bx0 = P.col0 >> 3;
    P.bz0 = P.row0 >> 3;
    P.nbx = ((P.col0 + P.cols - 1u) >> 3) - P.bx0 + 1u;
    P.nbz = ((P.row0 + P.rows - 1u) >> 3) - P.bz0 + 1u;
}

// first index in [lo, hi) whose level is > v (hi: none)
F3D_HD uint32_t contour_above(const float *levels, uint32_t lo, uint32_t hi, float v) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (levels[mid] > v) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// The wave: the levels that can cross block (bx, bz) of the cell grid, [lo, hi).
F3D_HD void contour_block_range(const ContourParams &P, uint32_t bx, uint32_t bz, uint32_t &lo, uint32_t &hi) {
    lo = 0u;
    hi = P.level_count;
    if (P.cull == 0u) return;
    const TerrainDev &T = P.terrain;
    const bool has3 = T.mip_count > 3u;
    const uint32_t level = has3 ? 3u : T.mip_count - 1u;
    const NodeRec band = T.bands[T.band_offset[level] + (has3 ? (bz << T.band_shift[level]) + bx : 0u)];
    lo = contour_above(P.levels, 0u, P.level_count, band.mn);
    hi = contour_above(P.levels, lo, P.level_count, band.mx);
}

// The lane: its cell's levels inside the block's, [l0, l1).
F3D_HD void contour_lane_range(const ContourParams &P, const LeafRec &rec, uint32_t lo, uint32_t hi, uint32_t &l0, uint32_t &l1) {
    const float mn = f_min(f_min(rec.h00, rec.h10), f_min(rec.h01, rec.h11)), mx = f_max(f_max(rec.h00, rec.h10), f_max(rec.h01, rec.h11));
    l0 = contour_above(P.levels, lo, hi, mn);
    l1 = contour_above(P.levels, l0, hi, mx);
}

F3D_HD uint32_t contour_case(const LeafRec &rec, float level) {
    return (rec.h00 >= level ? 1u : 0u) | (rec.h10 >= level ? 2u : 0u) | (rec.h01 >= level ? 4u : 0u) | (rec.h11 >= level ? 8u : 0u);
}
F3D_HD uint32_t contour_case_segments(uint32_t c) { return (c == 0u || c == 15u) ? 0u : ((c == 6u || c == 9u) ? 2u : 1u); }

F3D_HD uint32_t contour_lane_count(const ContourParams &P, const LeafRec &rec, uint32_t l0, uint32_t l1) {
    uint32_t n = 0u;
    for (uint32_t k = l0; k < l1; k++) n += contour_case_segments(contour_case(rec, P.levels[k]));
    return n;
}

// the crossing's coordinate along its edge, from the sample of lower index `a`
F3D_HD float contour_along(float origin, uint32_t a, float spacing, float ha, float hb, float level) {
    const float t = (level - ha) / (hb - ha);
    if (t == 0.0f) return plane_at(origin, a, spacing);
    if (t == 1.0f) return plane_at(origin, a + 1u, spacing);
    return plane_at(origin, a, spacing) + t * spacing;
}

// the crossing of `level` on edge e of cell (cx, cz)
F3D_HD void contour_crossing(const TerrainDev &T, uint32_t cx, uint32_t cz, const LeafRec &rec, uint32_t e, float level, float &x, float &z) {
    if (e == kContourB || e == kContourT) {
        const bool top = e == kContourT;
        x = contour_along(T.origin_x, cx, T.spacing_x, top ? rec.h01 : rec.h00, top ? rec.h11 : rec.h10, level);
        z = plane_at(T.origin_z, cz + (top ? 1u : 0u), T.spacing_z);
    } else {
        const bool right = e == kContourR;
        x = plane_at(T.origin_x, cx + (right ? 1u : 0u), T.spacing_x);
        z = contour_along(T.origin_z, cz, T.spacing_z, right ? rec.h10 : rec.h00, right ? rec.h11 : rec.h01, level);
    }
}

// The lane's segments, each given to f(at, ax, az, bx, bz, level index) with `at` counting up from the lane's offset.
template <class F>
F3D_HD void contour_lane_emit(const ContourParams &P, uint32_t cx, uint32_t cz, const LeafRec &rec, uint32_t l0, uint32_t l1, uint64_t at, F &&f) {
    for (uint32_t k = l0; k < l1; k++) {
        const float level = P.levels[k];
        const uint32_t c = contour_case(rec, level), n = contour_case_segments(c);
        for (uint32_t s = 0u; s < n; s++) {
            const uint32_t code = s == 0u ? (uint32_t)(kContourFirst >> (4u * c)) & 15u : (c == 6u ? kContourSecond6 : kContourSecond9);
            float ax, az, bx, bz;
            contour_crossing(P.terrain, cx, cz, rec, code & 3u, level, ax, az);
            contour_crossing(P.terrain, cx, cz, rec, code >> 2, level, bx, bz);
            f(at, ax, az, bx, bz, k);
            at++;
        }
    }
}

// The record a segment becomes in the paint form.
F3D_HD PaintPrim contour_prim(const float rgba[4], float ax, float az, float bx, float bz) {
    PaintPrim p;
    p.v[0] = ax, p.v[1] = az, p.v[2] = bx, p.v[3] = bz, p.v[4] = bx, p.v[5] = bz;
    for (uint32_t k = 0u; k < 12u; k++) p.c[k] = rgba[k & 3u];
    p.feature = 0u;
    p.reserved = 0u;
    return p;
}

#if defined(__HIPCC__)
// ... and how the emit kernels (f3d_contour.hip, f3d_drainage.hip) write it: a record is 80 bytes in a buffer aligned to 256,
// five 16-byte stores.
__device__ __forceinline__ void contour_prim_store(PaintPrim *dst, const PaintPrim &p) {
    uint4 words[kPaintPrimWords / 4u];
    __builtin_memcpy(words, &p, sizeof p);
    for (uint32_t k = 0u; k < kPaintPrimWords / 4u; k++) ((uint4 *)dst)[k] = words[k];
}
#endif

// lane -> cell of block (bx, bz); false: outside the region
F3D_HD bool contour_lane_cell(const ContourParams &P, uint32_t bx, uint32_t bz, uint32_t lane, uint32_t &cx, uint32_t &cz) {
    cx = (bx << 3) + (lane & 7u);
    cz = (bz << 3) + (lane >> 3);
    return cx >= P.col0 && cx - P.col0 < P.cols && cz >= P.row0 && cz - P.row0 < P.rows;
}

// What both passes share, per lane of the wave that owns block `block` of the region's blocks: the lane's cell, record and
// level range, and its count (0 for a lane outside the region).  false: no level can cross the block -- the same answer in
// every lane of the wave, which retires.
struct ContourLane {
    uint32_t cx, cz, l0, l1, n;
    LeafRec rec;
};
F3D_HD bool contour_lane(const ContourParams &P, uint32_t block, uint32_t lane, ContourLane &L) {
    const uint32_t bz = P.bz0 + block / P.nbx, bx = P.bx0 + block % P.nbx;
    uint32_t lo, hi;
    contour_block_range(P, bx, bz, lo, hi);  // (wave-uniform: the block's band and the bisection are scalar work on the device)
    L.n = 0u;
    L.l0 = L.l1 = 0u;
    if (lo >= hi) return false;
    if (contour_lane_cell(P, bx, bz, lane, L.cx, L.cz)) {
        L.rec = P.terrain.leaves[tiled_index(L.cx, L.cz, P.terrain.tiles_x[0])];
        contour_lane_range(P, L.rec, lo, hi, L.l0, L.l1);
        L.n = contour_lane_count(P, L.rec, L.l0, L.l1);
    }
    return true;
}

}  // namespace f3d
