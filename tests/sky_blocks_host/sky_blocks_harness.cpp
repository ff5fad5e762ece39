// tests/sky_blocks_host/sky_blocks_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_sky_blocks_host.py compiles and runs it).
//
// The deep-sky block rule (forge3d_amd/csrc/f3d_skyblocks.h) on the host: the text k_sky_blocks classifies a block with and
// the text the frame kernels find a tile's block with.
//
//   sky_blocks_harness classify   stdin: cases "width height row_begin row_end mask", mask = (row_end - row_begin) x width
//                                 characters '0' / '1' (row-major over the owned rows: does the pixel hold the sky
//                                 certificate); stdout: per case one line, a character '0' / '1' per block: is it deep --
//                                 the AND over the 64 lanes of sky_block_lane_clear, as the kernel's ballot takes it
//   sky_blocks_harness nest       every (width 1..40, rows 1..40, S 1 / 2 / 4 / 8): each tile of the band lies in exactly
//                                 one block, the one sky_block_of_tile names, and a tile of S = 1 IS its block
//
// Built as a program (its own main; may be built with -fsanitize=address,undefined).  The first failed check ends it with a
// non-zero status.
#include "../../forge3d_amd/csrc/f3d_skyblocks.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace f3d;

namespace {

int classify() {
    std::vector<char> mask;
    std::string line;
    unsigned width, height, row_begin, row_end;
    size_t cases = 0;
    while (scanf("%u %u %u %u", &width, &height, &row_begin, &row_end) == 4) {
        if (width == 0u || row_begin >= row_end || row_end > height) {
            fprintf(stderr, "FAILED case %zu: bad geometry %u %u %u %u\n", cases, width, height, row_begin, row_end);
            return 1;
        }
        const size_t n = (size_t)(row_end - row_begin) * width;
        mask.assign(n, 0);
        for (size_t i = 0; i < n; i++) {
            int c;
            do c = getchar(); while (c == ' ' || c == '\n');
            if (c != '0' && c != '1') {
                fprintf(stderr, "FAILED case %zu: mask character %d at %zu\n", cases, c, i);
                return 1;
            }
            mask[i] = (char)(c == '1');
        }
        const SkyBlockGeom g{width, height, row_begin, row_end};
        const TileGrid grid = sky_block_grid(g);
        line.assign(grid.count(), '0');
        for (uint32_t b = 0; b < grid.count(); b++) {
            bool deep = true;
            for (uint32_t lane = 0; lane < 64u; lane++) {
                // std::vector::at: a sample the rule sends outside the owned rows or the image would throw here
                const bool clear = sky_block_lane_clear(g, b, lane, [&](uint32_t x, uint32_t y) {
                    if (x >= width || y < row_begin || y >= row_end) {
                        fprintf(stderr, "FAILED case %zu: block %u looks up (%u, %u), which the strip does not own\n", cases, b, x, y);
                        exit(1);
                    }
                    return mask.at((size_t)(y - row_begin) * width + x) != 0;
                });
                deep = deep && clear;
            }
            line[b] = deep ? '1' : '0';
        }
        puts(line.c_str());
        cases++;
    }
    fprintf(stderr, "classify: %zu cases\n", cases);
    return 0;
}

int nest() {
    size_t cases = 0;
    for (uint32_t width = 1; width <= 40u; width++)
        for (uint32_t rows = 1; rows <= 40u; rows++)
            for (uint32_t lanes : {1u, 2u, 4u, 8u}) {
                const TileDims d = tile_shape(lanes);
                const TileGrid tiles = tile_grid(width, rows, d), blocks = tile_grid(width, rows, kSkyBlockShape);
                if (sky_block_grid(SkyBlockGeom{width, rows + 7u, 3u, 3u + rows}).count() != blocks.count()) {
                    fprintf(stderr, "FAILED width %u rows %u: the block grid is not the band's 8 x 8 tiling\n", width, rows);
                    return 1;
                }
                for (uint32_t t = 0; t < tiles.count(); t++) {
                    const uint32_t block = sky_block_of_tile(t, tiles.tiles_x, d, blocks.tiles_x);
                    if (block >= blocks.count() || (lanes == 1u && block != t)) {
                        fprintf(stderr, "FAILED width %u rows %u lanes %u tile %u: block %u of %u\n", width, rows, lanes, t, block, blocks.count());
                        return 1;
                    }
                    for (uint32_t lane = 0; lane < 64u; lane++) {
                        uint32_t gx, gy;
                        tile_lane_pixel(t, lane, tiles.tiles_x, 0u, d, gx, gy);
                        // every pixel the tile's lanes produce -- inside the band or past its ragged edge -- lies in the
                        // block's own 8 x 8 pixels: no tile straddles two blocks
                        if (gx / 8u != block % blocks.tiles_x || gy / 8u != block / blocks.tiles_x) {
                            fprintf(stderr, "FAILED width %u rows %u lanes %u tile %u lane %u: pixel (%u, %u) is not in block %u\n", width, rows,
                                    lanes, t, lane, gx, gy, block);
                            return 1;
                        }
                    }
                }
                cases++;
            }
    printf("nest: %zu cases\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "classify")) return classify();
    if (argc == 2 && !strcmp(argv[1], "nest")) return nest();
    fprintf(stderr, "usage: sky_blocks_harness classify | nest\n");
    return 2;
}
