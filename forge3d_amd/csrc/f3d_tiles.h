// forge3d_amd/csrc/f3d_tiles.h -- the tile geometry of the frame path, for the device and the host alike: the ONE definition
// of a wave's pixel tile, of the tile grid of a band, of the launch size and of which workgroup renders which tile.  The
// kernels (f3d_frame.h tile_pixel / lane_pixel), the launchers (f3d_kernels.hip), the row costs (f3d_host.hip) and
// tests/tiles_host run this text; it has no HIP built-ins.
#pragma once

#include "f3d_math.h"

namespace f3d {

constexpr int kNumXcd = 8;
constexpr uint32_t kNoTile = 0xFFFFFFFFu;  // a workgroup without a tile: padding of the launch

// Pixel tile of a wave with S sample lanes per pixel: 64 / S pixels, TW x TH.
template <uint32_t S>
struct TileShape {
    static constexpr uint32_t kLogS = S == 1u ? 0u : (S == 2u ? 1u : (S == 4u ? 2u : 3u));
#if defined(F3D_TILE_LOGW_S4)  // A/B of the tile shape (profiles/README.md)
    static constexpr uint32_t kLogW = S <= 2u ? 3u : (S == 4u ? F3D_TILE_LOGW_S4 : 2u);
#else
    static constexpr uint32_t kLogW = S <= 2u ? 3u : 2u;      // 8, 8, 4, 4 pixels wide
#endif
    static constexpr uint32_t kLogH = 6u - kLogS - kLogW;     // 8, 4, 4, 2 pixels high
};

// The same as a value, for code that learns the lane count at run time (any count but 1, 2, 4: the 8-lane tile).
struct TileDims {
    uint32_t log_s, log_w, log_h;
    F3D_HD constexpr uint32_t width() const { return 1u << log_w; }
    F3D_HD constexpr uint32_t height() const { return 1u << log_h; }
};
template <uint32_t S>
F3D_HD constexpr TileDims tile_shape() { return TileDims{TileShape<S>::kLogS, TileShape<S>::kLogW, TileShape<S>::kLogH}; }
F3D_HD constexpr TileDims tile_shape(uint32_t lanes) {
    return lanes == 1u ? tile_shape<1u>() : (lanes == 2u ? tile_shape<2u>() : (lanes == 4u ? tile_shape<4u>() : tile_shape<8u>()));
}
template <uint32_t S>
F3D_HD constexpr bool is_tile_shape(TileDims d) {
    return d.log_s == TileShape<S>::kLogS && d.log_w == TileShape<S>::kLogW && d.log_h == TileShape<S>::kLogH;
}
static_assert(is_tile_shape<1u>(tile_shape(1u)), "the run-time twin is TileShape<1>");
static_assert(is_tile_shape<2u>(tile_shape(2u)), "the run-time twin is TileShape<2>");
static_assert(is_tile_shape<4u>(tile_shape(4u)), "the run-time twin is TileShape<4>");
static_assert(is_tile_shape<8u>(tile_shape(8u)), "the run-time twin is TileShape<8>");

// Tiles of a band of `rows` image rows, tiled from its first row: tile t is column t % tiles_x of tile row t / tiles_x.
struct TileGrid {
    uint32_t tiles_x, tiles_y;
    F3D_HD constexpr uint32_t count() const { return tiles_x * tiles_y; }
};
F3D_HD constexpr uint32_t tiles_across(uint32_t width, TileDims d) { return (width + (d.width() - 1u)) >> d.log_w; }
F3D_HD constexpr uint32_t tiles_down(uint32_t rows, TileDims d) { return (rows + (d.height() - 1u)) >> d.log_h; }
F3D_HD constexpr TileGrid tile_grid(uint32_t width, uint32_t rows, TileDims d) { return TileGrid{tiles_across(width, d), tiles_down(rows, d)}; }

// Workgroup b is observed to run on XCD b % 8.  tile_map picks how tiles are dealt to XCDs:
//   1  tile id = workgroup id (consecutive tiles on different XCDs)
//   2  tile ROWS dealt round-robin to XCDs (row r -> XCD r % 8) -- the default: the load
//      balance of 1 with each XCD's L2 still seeing whole rows of coherent rays
//   3  contiguous image bands per XCD (best L2 locality, but a sky band idles its XCD:
//      measured 1.77x slower on the headline scene)
// Workgroups of a launch: every XCD gets as many, so some are padding.  Workgroups [0, launch_size) reach every tile
// exactly once (workgroup_tile); 0: an empty band.
F3D_HD constexpr uint32_t launch_size(TileGrid g, uint32_t tile_map) {
    if (g.tiles_y == 0u) return 0u;
    if (tile_map == 2u) return ((g.tiles_y + kNumXcd - 1u) / kNumXcd) * g.tiles_x * kNumXcd;
    return ((g.count() + kNumXcd - 1u) / kNumXcd) * kNumXcd;
}
// Tile of workgroup wg (its position in the dispatch order of one frame) into `tile`; false, and kNoTile: the workgroup is
// padding.  `order` (map 2 only): the same row -> XCD dealing, but each XCD starts its most expensive tiles first
// (f3d_frame.h k_tile_order; its padding entries are kNoTile).
F3D_HD bool workgroup_tile(uint32_t wg, TileGrid g, uint32_t tile_map, const uint32_t *order, uint32_t &tile) {
    const uint32_t tiles_x = g.tiles_x, tiles_y = g.tiles_y, ntiles = tiles_x * tiles_y;
    tile = kNoTile;
    uint32_t t;
    if (order) {
        t = order[wg];
    } else if (tile_map == 1u) {
        t = wg;
    } else if (tile_map == 2u) {
        const uint32_t xcd = wg % kNumXcd, i = wg / kNumXcd;
        const uint32_t rows_per_xcd = (tiles_y + kNumXcd - 1u) / kNumXcd;
        const uint32_t ty = (i / tiles_x) * kNumXcd + xcd;
        if (i >= rows_per_xcd * tiles_x || ty >= tiles_y) return false;
        t = ty * tiles_x + (i % tiles_x);
    } else {  // 3 (and anything else): contiguous bands
        const uint32_t per_xcd = (ntiles + kNumXcd - 1u) / kNumXcd;
        t = (wg % kNumXcd) * per_xcd + wg / kNumXcd;
    }
    if (t >= ntiles) return false;
    tile = t;
    return true;
}
// Pixel of lane `lane` of the wave that renders `tile`: the S sample lanes of a pixel are neighbours.  Lanes of a ragged
// tile get coordinates outside the image (gx >= width) or below the band.
F3D_HD void tile_lane_pixel(uint32_t tile, uint32_t lane, uint32_t tiles_x, uint32_t band_begin, TileDims d, uint32_t &gx, uint32_t &gy) {
    const uint32_t pixel = lane >> d.log_s;
    gx = (tile % tiles_x) * d.width() + (pixel & (d.width() - 1u));
    gy = band_begin + (tile / tiles_x) * d.height() + (pixel >> d.log_w);
}

// Per-tile costs of a strip of `rows` rows spread over its image rows: a tile's cost goes to its rows in equal parts (the
// last tile row may be ragged).  Every row of a tile row gets the same sum, accumulated in double in ascending tile id.
inline void spread_tile_costs(const uint32_t *cost, uint32_t width, uint32_t rows, TileDims d, float *out) {
    const TileGrid g = tile_grid(width, rows, d);
    for (uint32_t ty = 0; ty < g.tiles_y; ty++) {
        const uint32_t r0 = ty * d.height(), r1 = rows < r0 + d.height() ? rows : r0 + d.height();
        double sum = 0.0;
        for (uint32_t tx = 0; tx < g.tiles_x; tx++) sum += (double)cost[ty * g.tiles_x + tx] / (double)(r1 - r0);
        for (uint32_t r = r0; r < r1; r++) out[r] = (float)sum;
    }
}

}  // namespace f3d
