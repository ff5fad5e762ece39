// tests/emul/direct_levels.h -- TEST INFRASTRUCTURE ONLY (the raster walks' host harnesses include it after host_scene.h).
// The Levels adapter of the raster walks (csrc/f3d_walk.h pyramid_walk) on the host: the terrain's own per-level layout.
#pragma once

namespace {
struct DirectLevels {
    void band_entry(const TerrainDev &T, uint32_t level, uint32_t &offset, uint32_t &shift) const {
        offset = T.band_offset[level];
        shift = T.band_shift[level];
    }
};
}  // namespace
