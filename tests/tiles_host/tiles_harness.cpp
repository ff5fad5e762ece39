// tests/tiles_host/tiles_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_tiles_host.py compiles and runs it).
//
// The tile geometry of the frame path (forge3d_amd/csrc/f3d_tiles.h) on the host: the text the kernels run (tile_pixel /
// lane_pixel call it) and the text the launchers size their grids and buffers with, checked against each other.
//
//   tiles_harness check    every (width 1..33, band rows 0..17, band_begin 0 / 5, S 1 / 2 / 4 / 8, tile map 1 / 2 / 3): the
//                          launch reaches every tile once, the tiles and their lanes every pixel of the band S times
//   tiles_harness spread   stdin: cases "width rows lanes cost[0] ... cost[tiles - 1]"; stdout: per case one line, the row
//                          costs of spread_tile_costs as float bits (hexadecimal)
//
// Built as a program (its own main; may be built with -fsanitize=address,undefined).  The first failed check ends it with a
// non-zero status.
#include "../../forge3d_amd/csrc/f3d_tiles.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace f3d;

namespace {

struct Case {
    uint32_t width, rows, band_begin, lanes, tile_map;
};

[[noreturn]] void fail(const Case &c, const char *what, long long a = 0, long long b = 0) {
    fprintf(stderr, "FAILED width %u rows %u band_begin %u lanes %u tile_map %u: %s (%lld, %lld)\n", c.width, c.rows, c.band_begin,
            c.lanes, c.tile_map, what, a, b);
    exit(1);
}

void check(const Case &c) {
    const TileDims d = tile_shape(c.lanes);
    const bool twin = c.lanes == 1u ? is_tile_shape<1u>(d) : c.lanes == 2u ? is_tile_shape<2u>(d) : c.lanes == 4u ? is_tile_shape<4u>(d) : is_tile_shape<8u>(d);
    if (!twin) fail(c, "tile_shape(lanes) is not TileShape<S>");
    if ((1u << d.log_s) != c.lanes || d.width() * d.height() * c.lanes != 64u) fail(c, "a tile is not 64 / S pixels", d.width(), d.height());

    const uint32_t band_end = c.band_begin + c.rows;
    const TileGrid g = tile_grid(c.width, c.rows, d);
    const uint32_t across = (c.width + d.width() - 1u) / d.width(), down = (c.rows + d.height() - 1u) / d.height();  // plain division
    if (g.tiles_x != across || g.tiles_y != down) fail(c, "tiles_x / tiles_y", g.tiles_x, g.tiles_y);
    if (g.count() != across * down) fail(c, "tile count is not tiles_x * tiles_y", g.count(), across * down);

    const uint32_t launch = launch_size(g, c.tile_map);
    if ((launch == 0u) != (c.rows == 0u)) fail(c, "the grid is empty exactly when the band is", launch);
    if (launch % 8u != 0u) fail(c, "the grid is not a multiple of 8", launch);
    if (launch < g.count()) fail(c, "fewer workgroups than tiles", launch, g.count());

    // workgroups [0, launch) -> tiles [0, count) one-to-one; every other workgroup is padding.  An order that lists what
    // the map gives (as k_tile_order's does, up to a permutation inside each XCD) is read the same way.
    std::vector<uint32_t> reached(g.count(), 0u), listed(launch);
    uint32_t padding = 0u;
    for (uint32_t wg = 0; wg < launch; wg++) {
        uint32_t tile = 12345u;
        const bool real = workgroup_tile(wg, g, c.tile_map, nullptr, tile);
        listed[wg] = tile;
        if (real != (tile != kNoTile)) fail(c, "a workgroup's verdict and its tile disagree", wg, tile);
        if (!real) {
            padding++;
            continue;
        }
        if (tile >= g.count()) fail(c, "a workgroup's tile is no tile", wg, tile);
        if (reached[tile]++) fail(c, "two workgroups reach one tile", wg, tile);
    }
    if (padding != launch - g.count()) fail(c, "tiles left without a workgroup", padding, launch - g.count());
    for (uint32_t wg = 0; wg < launch; wg++) {
        uint32_t tile = 12345u;
        const bool real = workgroup_tile(wg, g, c.tile_map, listed.data(), tile);
        if (tile != listed[wg] || real != (tile != kNoTile)) fail(c, "a tile order is not read as it was written", wg, tile);
    }

    // all tiles x 64 lanes: every pixel of the band S times, by S consecutive lanes; whatever else is produced lies right
    // of the image or below the band
    std::vector<uint32_t> produced((size_t)c.width * c.rows, 0u);
    for (uint32_t tile = 0; tile < g.count(); tile++) {
        uint32_t first_x = 0u, first_y = 0u;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t gx = 0xdeadu, gy = 0xdeadu;
            tile_lane_pixel(tile, lane, g.tiles_x, c.band_begin, d, gx, gy);
            if (lane % c.lanes == 0u) {
                first_x = gx;
                first_y = gy;
            } else if (gx != first_x || gy != first_y) {
                fail(c, "the sample lanes of a pixel are not consecutive lanes", tile, lane);
            }
            if (gy < c.band_begin) fail(c, "a pixel above the band", gx, gy);
            if (gx < c.width && gy < band_end) produced[(size_t)(gy - c.band_begin) * c.width + gx]++;
            else if (!(gx >= c.width || gy >= band_end)) fail(c, "a pixel outside the band that is neither right of the image nor below the band", gx, gy);
        }
    }
    for (size_t i = 0; i < produced.size(); i++)
        if (produced[i] != c.lanes) fail(c, "a pixel of the band is not produced S times", (long long)i, produced[i]);
}

int check_all() {
    unsigned long long cases = 0;
    for (uint32_t width = 1; width <= 33u; width++)
        for (uint32_t rows = 0; rows <= 17u; rows++)
            for (uint32_t band_begin : {0u, 5u})
                for (uint32_t lanes : {1u, 2u, 4u, 8u})
                    for (uint32_t tile_map : {1u, 2u, 3u}) {
                        check(Case{width, rows, band_begin, lanes, tile_map});
                        cases++;
                    }
    printf("check: %llu cases\n", cases);
    return 0;
}

int spread() {
    uint32_t width, rows, lanes;
    unsigned long long cases = 0;
    while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &width, &rows, &lanes) == 3) {
        const TileDims d = tile_shape(lanes);
        std::vector<uint32_t> cost(tile_grid(width, rows, d).count());
        for (uint32_t &v : cost)
            if (scanf("%" SCNu32, &v) != 1) return 2;
        const float untouched = -1.0f;
        std::vector<float> out(rows, untouched);
        spread_tile_costs(cost.data(), width, rows, d, out.data());
        for (uint32_t r = 0; r < rows; r++) {
            uint32_t bits;
            memcpy(&bits, &out[r], 4);
            printf(r ? " %08x" : "%08x", bits);
        }
        printf("\n");
        cases++;
    }
    fprintf(stderr, "spread: %llu cases\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "check")) return check_all();
    if (argc >= 2 && !strcmp(argv[1], "spread")) return spread();
    fprintf(stderr, "usage: tiles_harness check | spread < cases\n");
    return 2;
}
