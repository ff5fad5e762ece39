// forge3d_amd/csrc/f3d_skyblocks.h -- deep-sky blocks, for the device and the host alike: which 8 x 8 pixel blocks of a
// strip lie so far inside certified sky that no frame can change anything of theirs but the accumulation.
// The kernel that builds the table (f3d_frame.h k_sky_blocks), the kernels that read it (k_head, frame_wave), the host's
// diagnostic (f3d_host.hip f3d_session_sky_blocks) and tests/sky_blocks_host run this text; it has no HIP built-ins.
//
// A BLOCK is a tile of TileShape<1> -- the tile of a k_head wave -- of the strip's tiling from its first owned row: block b
// is column b % blocks_x of block row b / blocks_x.  The 8 x 4, 4 x 4 and 4 x 2 tiles of the sample-lane frame kernels nest
// inside it (sky_block_of_tile).
//
// A block is DEEP when every pixel of its rectangle [x0 - 4, x0 + 12) x [y0 - 4, y0 + 12) holds the sky certificate
// (f3d_cone.h certified_sky), where
//   * a pixel outside the image counts as holding it: the spatial pass clamps its reach to the image;
//   * a row inside the image that the strip does not own counts as NOT holding it: a strip knows nothing of its
//     neighbours' certificates.
// The margin is 4 on every side; the spatial pass reaches -3 ... +4 (f3d_scene.h kSpatialReachLo / kSpatialReachHi), so the
// rounder rule is conservative: every reservoir a deep block's head could read, and every reservoir whose head could read
// a deep block's, belongs to a certified pixel.
#pragma once

#include "f3d_tiles.h"

namespace f3d {

constexpr uint32_t kSkyBlockMargin = 4u;
// A block's word in the table: bit 0 = deep; the bits from kSkyBlockCountShift on are the table builder's count of the
// block's own certified pixels (a diagnostic: no frame reads it).
constexpr uint32_t kSkyBlockDeep = 1u, kSkyBlockCountShift = 8u;
constexpr TileDims kSkyBlockShape = tile_shape<1u>();
static_assert(kSkyBlockShape.log_w == 3u && kSkyBlockShape.log_h == 3u, "a block is 8 x 8 pixels");
constexpr uint32_t kSkyBlockSpan = 8u + 2u * kSkyBlockMargin;  // the rectangle's side: 16 pixels
static_assert(kSkyBlockSpan * kSkyBlockSpan == 4u * 64u, "a wave looks at the rectangle in four rounds of 64 lanes");

// The strip a table belongs to: the image and the rows it owns.
struct SkyBlockGeom {
    uint32_t width, height;       // the image
    uint32_t row_begin, row_end;  // owned rows; blocks tile them from row_begin
};
F3D_HD constexpr TileGrid sky_block_grid(const SkyBlockGeom &g) { return tile_grid(g.width, g.row_end - g.row_begin, kSkyBlockShape); }

// Sample k (0 ... 255, row-major over the 16 x 16 rectangle) of block `block`: what it says by its position alone.
//   kSkySampleOutside  outside the image: counts as certified
//   kSkySampleForeign  inside the image, in a row of another strip: not certified
//   kSkySampleLookUp   pixel (x, y) of the strip: its certificate decides
constexpr uint32_t kSkySampleOutside = 0u, kSkySampleForeign = 1u, kSkySampleLookUp = 2u;
F3D_HD uint32_t sky_block_sample(const SkyBlockGeom &g, uint32_t block, uint32_t k, uint32_t &x, uint32_t &y) {
    const uint32_t blocks_x = tiles_across(g.width, kSkyBlockShape);
    // (signed: the rectangle of a block on the image's rim starts before column / row 0)
    const int sx = (int)((block % blocks_x) * 8u) - (int)kSkyBlockMargin + (int)(k % kSkyBlockSpan);
    const int sy = (int)(g.row_begin + (block / blocks_x) * 8u) - (int)kSkyBlockMargin + (int)(k / kSkyBlockSpan);
    x = (uint32_t)sx;
    y = (uint32_t)sy;
    if (sx < 0 || sy < 0 || sx >= (int)g.width || sy >= (int)g.height) return kSkySampleOutside;
    if (y < g.row_begin || y >= g.row_end) return kSkySampleForeign;
    return kSkySampleLookUp;
}

// Lane `lane` of the wave that classifies `block`: do its four samples leave the block deep?  certified(x, y): does owned
// pixel (x, y) hold the sky certificate.  The block is deep when all 64 lanes say yes.
template <class Certified>
F3D_HD bool sky_block_lane_clear(const SkyBlockGeom &g, uint32_t block, uint32_t lane, Certified &&certified) {
    bool clear = true;
    for (uint32_t i = 0u; i < 4u; i++) {
        uint32_t x, y;
        const uint32_t where = sky_block_sample(g, block, lane + 64u * i, x, y);
        if (where == kSkySampleForeign) clear = false;
        else if (where == kSkySampleLookUp && !certified(x, y)) clear = false;
    }
    return clear;
}

// The block that holds tile `tile` of a band tiled with `d` from the strip's first row (one band: the strip's own tiling).
F3D_HD uint32_t sky_block_of_tile(uint32_t tile, uint32_t tiles_x, TileDims d, uint32_t blocks_x) {
    const uint32_t px = (tile % tiles_x) << d.log_w, py = (tile / tiles_x) << d.log_h;
    return (py >> 3) * blocks_x + (px >> 3);
}

}  // namespace f3d
