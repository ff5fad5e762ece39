// forge3d_amd/csrc/f3d_retable.h -- the acceleration tables of a live session patched under new DEM samples
// (f3d_session_reterrain).
//
// build_tables (f3d_host_mem.h) makes the tables of a whole DEM from a raw-height buffer through a tiled node table, one
// launch per level and a second one per band level.  A session that re-terrains owns its leaf table and its band tables
// (TableLayout sizes; the scene-cache entry other sessions share is never written) and patches them from a BLOCK of new
// samples -- bw x bh at sample (x0, y0); the whole DEM is the block (0, 0, w, h) -- without a raw-height copy and without a
// node table:
//   leaf      the cells [max(x0,1)-1, min(x0+bw-1, cell_w-1)] x (the same in y) are the ones with a corner in the block: the
//             DIRTY range.  A cell's record is read, exactly the corners inside the block are replaced by
//             height * exaggeration (leaf_build_at's product, so its bits), and written back with its level-0 band
//             (min4, max4).  Records hold h * exaggeration: a corner outside the block is kept, not recomputed.
//   levels    band level l from band level l - 1 over [lo >> l, hi >> l]: level_build_at's 2x2 order, its clamp-to-edge
//             once an axis has collapsed, its skip of level-0 children outside the cell grid; a child ROW the band tables
//             do not store (band_rows: it holds no cell) is (+inf, -inf), which is what the node table holds there.
//             The operations and their order are the builders', so the bits are -- signed zeros included.
// Nothing outside the dirty range is written.  Two launches whatever the DEM's size (f3d_retable.hip):
//   k_retable_tiles   one workgroup per aligned 64x64-cell tile of the dirty range: leaves patched, levels 0..6 reduced in LDS
//   k_retable_top     ONE workgroup walks the levels above through global memory, a barrier between levels
// The per-thread bodies below are host-and-device: tests/reterrain_host runs them on the CPU in a shuffled thread order.
#pragma once

#include "f3d_setup.h"

namespace f3d {

constexpr uint32_t kRetableTile = 64u;      // cells per side of a tile workgroup's tile
constexpr uint32_t kRetableTileLevels = 7u;  // levels 0..6 live in its LDS: 64^2 + 32^2 + ... + 1 records
constexpr uint32_t kRetableTileRecords = 5461u;

struct RetableParams {
    const float *block;      // the new samples, row-major, pitch bw (device)
    uint32_t x0, y0, bw, bh;  // DEM sample of the block's first sample, the block's size
    float exaggeration;
    LeafRec *leaves;         // the session's own tables
    NodeRec *bands;
    uint32_t leaf_tiles_x;
    uint32_t cell_w, cell_h;
    uint32_t levels;
    uint32_t level_w[kMaxLevels], level_h[kMaxLevels];  // logical pow2 dims
    uint32_t band_offset[kMaxLevels], band_shift[kMaxLevels], band_rows[kMaxLevels];
    uint32_t lo_x, lo_y, hi_x, hi_y;  // dirty cells, inclusive
    uint32_t tile_x0, tile_y0, tiles_x, tiles_y;  // the tiles the dirty range touches: first one, count per axis
};

// dirty range and tile range of a block (the block lies inside the w x h DEM, bw, bh >= 1)
inline RetableParams retable_params(const TableLayout &L, const float *block, uint32_t x0, uint32_t y0, uint32_t bw, uint32_t bh,
                                    float exaggeration, LeafRec *leaves, NodeRec *bands) {
    RetableParams P{};
    P.block = block;
    P.x0 = x0, P.y0 = y0, P.bw = bw, P.bh = bh;
    P.exaggeration = exaggeration;
    P.leaves = leaves;
    P.bands = bands;
    P.leaf_tiles_x = L.tiles_x[0];
    P.cell_w = L.cell_w, P.cell_h = L.cell_h;
    P.levels = L.levels;
    for (uint32_t l = 0; l < kMaxLevels; l++) {
        P.level_w[l] = L.level_w[l], P.level_h[l] = L.level_h[l];
        P.band_offset[l] = L.band_offset[l], P.band_shift[l] = L.band_shift[l], P.band_rows[l] = L.band_rows[l];
    }
    P.lo_x = (x0 > 1u ? x0 : 1u) - 1u;
    P.lo_y = (y0 > 1u ? y0 : 1u) - 1u;
    P.hi_x = x0 + bw - 1u < L.cell_w - 1u ? x0 + bw - 1u : L.cell_w - 1u;
    P.hi_y = y0 + bh - 1u < L.cell_h - 1u ? y0 + bh - 1u : L.cell_h - 1u;
    P.tile_x0 = P.lo_x / kRetableTile, P.tile_y0 = P.lo_y / kRetableTile;
    P.tiles_x = P.hi_x / kRetableTile - P.tile_x0 + 1u;
    P.tiles_y = P.hi_y / kRetableTile - P.tile_y0 + 1u;
    return P;
}

F3D_HD bool retable_dirty(const RetableParams &P, uint32_t l, uint32_t x, uint32_t y) {
    return x >= (P.lo_x >> l) && x <= (P.hi_x >> l) && y >= (P.lo_y >> l) && y <= (P.hi_y >> l);
}
F3D_HD uint32_t retable_tile_offset(uint32_t l) {  // of level l inside a tile's LDS records: sum of (64 >> k)^2, k < l
    return (16384u - (16384u >> (2u * l))) / 3u;
}

// New sample at DEM sample (sx, sy) if it lies in the block, else `kept`
F3D_HD float retable_corner(const RetableParams &P, uint32_t sx, uint32_t sy, float kept) {
    if (sx < P.x0 || sx >= P.x0 + P.bw || sy < P.y0 || sy >= P.y0 + P.bh) return kept;
    return P.block[(size_t)(sy - P.y0) * P.bw + (sx - P.x0)] * P.exaggeration;
}

// Dirty cell (x, y): its record patched and written with its level-0 band; returns the band
F3D_HD NodeRec retable_leaf_at(const RetableParams &P, uint32_t x, uint32_t y) {
    const uint32_t i = tiled_index(x, y, P.leaf_tiles_x);
    LeafRec rec = P.leaves[i];
    rec.h00 = retable_corner(P, x, y, rec.h00);
    rec.h10 = retable_corner(P, x + 1u, y, rec.h10);
    rec.h01 = retable_corner(P, x, y + 1u, rec.h01);
    rec.h11 = retable_corner(P, x + 1u, y + 1u, rec.h11);
    P.leaves[i] = rec;
    const NodeRec band{min4(rec), max4(rec)};
    P.bands[P.band_offset[0] + ((size_t)y << P.band_shift[0]) + x] = band;
    return band;
}

// Node (x, y) of level l >= 1 (inside the logical level) from its children through `child(sx, sy)`: level_build_at
template <class Child>
F3D_HD NodeRec retable_reduce(const RetableParams &P, uint32_t l, uint32_t x, uint32_t y, Child &&child) {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    const uint32_t src_w = P.level_w[l - 1u], src_h = P.level_h[l - 1u];
    for (uint32_t dy = 0u; dy < 2u; dy++) {
        for (uint32_t dx = 0u; dx < 2u; dx++) {
            uint32_t sx = 2u * x + dx, sy = 2u * y + dy;
            sx = sx < src_w - 1u ? sx : src_w - 1u;
            sy = sy < src_h - 1u ? sy : src_h - 1u;
            if (l == 1u && !(sx < P.cell_w && sy < P.cell_h)) continue;
            const NodeRec s = child(sx, sy);
            mn = f_min(mn, s.mn);
            mx = f_max(mx, s.mx);
        }
    }
    return NodeRec{mn, mx};
}

// Record (x, y) of band level l as the node table would hold it: rows without cells are not stored
F3D_HD NodeRec retable_band_read(const RetableParams &P, uint32_t l, uint32_t x, uint32_t y) {
    if (y >= P.band_rows[l]) return NodeRec{__builtin_inff(), -__builtin_inff()};
    return P.bands[P.band_offset[l] + ((size_t)y << P.band_shift[l]) + x];
}

// ---- tile pass: workgroup `tile` (0 .. tiles_x * tiles_y), `lds` its kRetableTileRecords records ---------------------------
// level 0: item i of 4096 -- in the leaf table's own order (8x8 tiles, Z-order inside), so a wave reads consecutive records
F3D_HD void retable_tile_level0(const RetableParams &P, uint32_t tile, NodeRec *lds, uint32_t i) {
    const uint32_t ox = (P.tile_x0 + tile % P.tiles_x) * kRetableTile, oy = (P.tile_y0 + tile / P.tiles_x) * kRetableTile;
    const uint32_t t8 = i >> 6;
    const uint32_t lx = ((t8 & 7u) << 3) | (i & 1u) | ((i >> 1) & 2u) | ((i >> 2) & 4u);
    const uint32_t ly = ((t8 >> 3) << 3) | ((i >> 1) & 1u) | ((i >> 2) & 2u) | ((i >> 3) & 4u);
    const uint32_t x = ox + lx, y = oy + ly;
    NodeRec out{__builtin_inff(), -__builtin_inff()};
    if (x < P.cell_w && y < P.cell_h)
        out = retable_dirty(P, 0u, x, y) ? retable_leaf_at(P, x, y) : P.bands[P.band_offset[0] + ((size_t)y << P.band_shift[0]) + x];
    lds[ly * kRetableTile + lx] = out;
}
// level l in 1 .. 6: item i of (64 >> l)^2, from the tile's level l - 1 in LDS; dirty nodes go to the band table
F3D_HD void retable_tile_level(const RetableParams &P, uint32_t tile, NodeRec *lds, uint32_t l, uint32_t i) {
    const uint32_t n = kRetableTile >> l, shift = 6u - l;
    const uint32_t ox = ((P.tile_x0 + tile % P.tiles_x) * kRetableTile) >> l, oy = ((P.tile_y0 + tile / P.tiles_x) * kRetableTile) >> l;
    const uint32_t lx = i & (n - 1u), ly = i >> shift;
    const uint32_t x = ox + lx, y = oy + ly;
    if (x >= P.level_w[l] || y >= P.level_h[l]) return;
    const NodeRec *src = lds + retable_tile_offset(l - 1u);
    const NodeRec out = retable_reduce(P, l, x, y, [&](uint32_t sx, uint32_t sy) { return src[(sy - 2u * oy) * (2u * n) + (sx - 2u * ox)]; });
    lds[retable_tile_offset(l) + ly * n + lx] = out;
    if (retable_dirty(P, l, x, y)) P.bands[P.band_offset[l] + ((size_t)y << P.band_shift[l]) + x] = out;
}

// ---- top pass: level l >= 7, item k of its dirty range, from band level l - 1 in global memory -----------------------------
F3D_HD uint32_t retable_top_count(const RetableParams &P, uint32_t l) {
    return ((P.hi_x >> l) - (P.lo_x >> l) + 1u) * ((P.hi_y >> l) - (P.lo_y >> l) + 1u);
}
F3D_HD void retable_top_at(const RetableParams &P, uint32_t l, uint32_t k) {
    const uint32_t rw = (P.hi_x >> l) - (P.lo_x >> l) + 1u;
    const uint32_t x = (P.lo_x >> l) + k % rw, y = (P.lo_y >> l) + k / rw;
    const NodeRec out = retable_reduce(P, l, x, y, [&](uint32_t sx, uint32_t sy) { return retable_band_read(P, l - 1u, sx, sy); });
    P.bands[P.band_offset[l] + ((size_t)y << P.band_shift[l]) + x] = out;
}

#if defined(__HIPCC__)
// f3d_retable.hip: both passes on `stream` (always two launches: the top pass of a DEM of seven levels or fewer walks nothing)
hipError_t launch_retable(const RetableParams &P, hipStream_t stream);
#endif

}  // namespace f3d
