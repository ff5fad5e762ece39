// tests/umbra_host/umbra_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_umbra_host.py compiles it).
// The shadow-depth rasters' lane body (f3d_umbra.h umbra_sample / umbra_depth, what k_umbra runs per lane) on the host over the
// waves and lanes k_umbra is launched with (f3d_walk.h region_waves / region_sample, both footprints).  The walk has no wave
// primitive in it, so a wave is a plain loop over its lanes; the loop over the directions and the maximum are written as the
// kernel writes them (k_umbra keeps them in the kernel: f3d_frame.h says why).  `cap` (0: horizon_step_cap) injects a tiny step
// cap -- here only, the library has no such switch.  umbra_horizon_run is the horizon raster's lane body (f3d_horizon.h horizon_lane) over the same
// scene, for the cross-check of the two walks.
// With -DUMBRA_DRIVER the file is a stand-alone program (its own main) over two synthetic DEMs, for a sanitizer build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../emul/direct_levels.h"
#include "../../forge3d_amd/csrc/f3d_umbra.h"

namespace {
// (directions null: one direction, `sun` -- what SESSION_SUN hands the kernel)
void run_umbra(const TerrainDev &T, V3 sun, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint32_t count,
               const float *directions, float *depth, float *deepest, float *samples, uint32_t cap, uint32_t block) {
    UmbraParams R{};
    R.terrain = T;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.row0 = row0;
    R.col0 = col0;
    R.rows = rows;
    R.cols = cols;
    R.direction_count = count;
    R.step_cap = cap ? cap : horizon_step_cap(T);
    R.block = block;
    R.sun = sun;
    R.directions = (const float4 *)directions;
    const uint32_t total = rows * cols;
    const long waves = region_waves(rows, cols, block);
    const DirectLevels levels;
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++)
        for (uint32_t lane = 0, n, i, j; lane < 64u; lane++)
            if (region_sample(rows, cols, block, (uint32_t)wv, lane, n)) {
                const V3 g = umbra_sample(R, n, i, j);
                store_point(samples, n, g);
                float deep = 0.0f;
                for (uint32_t k = 0u; k < count; k++) {
                    const float4 direction = R.directions ? R.directions[k] : float4{R.sun.x, R.sun.y, R.sun.z, 0.0f};
                    const float L = umbra_depth(R, g, i, j, direction, levels);
                    if (depth) depth[(size_t)k * total + n] = L;
                    deep = f_max(deep, L);
                }
                if (deepest) deepest[n] = deep;
            }
}
}  // namespace

// info[0..8]: scene_create's nine (tests/emul/host_scene.h)
extern "C" void *umbra_scene_create(const f3d_terrain_ref_desc *d, float *info) { return scene_create(d, 1, info, 9u); }
extern "C" void umbra_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One shadow-depth raster as f3d_session_umbra's device form answers it (flags: 2 CURVED, 16 SESSION_SUN: directions null, count 1).
// depth (count x rows * cols), deepest (rows * cols) and samples (rows * cols x 3: the lattice points) may each be null.
extern "C" int umbra_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint32_t count,
                         const float *directions, float *depth, float *deepest, float *samples, uint32_t cap, uint32_t block) {
    const HostScene *S = (const HostScene *)scene;
    const bool sun = (flags & 16u) != 0u;
    if (sun != (directions == nullptr) || (sun && count != 1u)) return 1;
    if ((uintptr_t)directions % alignof(float4) != 0u) return 2;  // (read as float4: a NumPy allocation is aligned, an odd view is not)
    run_umbra(S->P.terrain, S->P.light.wi, flags, row0, col0, rows, cols, count, directions, depth, deepest, samples, cap, block);
    return 0;
}

// The horizon raster's lane body at `lift` over the whole DEM: horizon (count x rows * cols) for azimuths (count x 2).
extern "C" int umbra_horizon_run(void *scene, uint32_t flags, float lift, uint32_t count, const float *azimuths, float *horizon) {
    const TerrainDev &T = ((const HostScene *)scene)->P.terrain;
    if ((uintptr_t)azimuths % alignof(float2) != 0u) return 2;  // (read as float2)
    HorizonParams R{};
    R.terrain = T;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.rows = T.cell_h + 1u;
    R.cols = T.cell_w + 1u;
    R.lift = lift;
    R.azimuth_count = count;
    R.step_cap = horizon_step_cap(T);
    R.azimuths = (const float2 *)azimuths;
    R.horizon = horizon;
#pragma omp parallel for schedule(dynamic, 64)
    for (long n = 0; n < (long)(R.rows * R.cols); n++) horizon_lane(R, (uint32_t)n, DirectLevels{});
    return 0;
}

extern "C" uint32_t umbra_step_cap_of(void *scene) { return horizon_step_cap(((const HostScene *)scene)->P.terrain); }
extern "C" uint32_t umbra_desc_size() { return (uint32_t)sizeof(f3d_session_umbra_desc); }

#if defined(UMBRA_DRIVER)
// A 65 x 63 and a 5 x 3 synthetic DEM; directions low and high, along either axis, through lattice corners, level, descending,
// straight up and down, zero, non-finite, with w != 0; the session-sun form; curved and flat, both footprints, a region, a tiny
// cap: every path of the lane body.  Prints one checksum line; exit status 0.
int main() {
    double check = 0.0;
    unsigned long long nans = 0ull, infs = 0ull;
    const uint32_t shapes[2][2] = {{65u, 63u}, {5u, 3u}};
    for (const auto &shape : shapes) {
        const uint32_t w = shape[0], h = shape[1];
        HostTables t;
        TerrainDev T{};
        driver_terrain(w, h, t, T);
        const float nan = f_from_bits(0x7FC00000u);
        alignas(16) const float directions[] = {
            -0.70f, 0.09f, -0.70f, 0.0f,             // a low sun
            0.55f, 0.50f, -0.66f, 0.0f,              // a high one
            1.0f, 0.17f, 0.0f, 0.0f,                 // along x: rows of flat-axis walks
            0.0f, 0.34f, -1.0f, 0.0f,                // along z, backward
            T.spacing_x, 0.2f, T.spacing_z, 0.0f,    // the cell diagonal: through lattice corners
            -0.8f, 0.0f, 0.6f, 0.0f,                 // level
            0.6f, -0.05f, 0.8f, 0.0f,                // descending
            0.0f, 1.0f, 0.0f, 0.0f,                  // straight up
            0.0f, -1.0f, 0.0f, 0.0f,                 // straight down: +inf
            0.0f, 0.0f, 0.0f, 0.0f,                  // the device form's NaN planes: zero,
            nan, 0.3f, 0.5f, 0.0f,                   // non-finite,
            0.5f, 0.3f, 0.5f, 1.0f,                  // w != 0
        };
        const uint32_t count = (uint32_t)(sizeof(directions) / sizeof(float)) / 4u, bad_from = count - 3u;
        const V3 sun{0.41f, 0.37f, -0.83f};
        for (uint32_t flags : {0u, 2u})
            for (uint32_t block : {0u, 1u})
                for (uint32_t cap : {0u, 3u}) {
                    const uint32_t row0 = block ? 1u : 0u, col0 = block ? 2u : 0u, rows = h - row0, cols = w - col0;
                    std::vector<float> planes((size_t)count * rows * cols), deep((size_t)rows * cols), samples((size_t)rows * cols * 3u);
                    run_umbra(T, sun, flags, row0, col0, rows, cols, count, directions, planes.data(), deep.data(), samples.data(), cap, block);
                    for (size_t q = 0; q < planes.size(); q++) {
                        const float v = planes[q];
                        if (v != v) nans += (cap || q / ((size_t)rows * cols) >= bad_from) ? 0ull : 1ull;
                        else if (std::isfinite(v)) check += v;
                        else infs++;
                    }
                    for (float v : deep)
                        if (std::isfinite(v)) check += v;
                    std::vector<float> one((size_t)rows * cols);
                    run_umbra(T, sun, flags | 16u, row0, col0, rows, cols, 1u, nullptr, one.data(), nullptr, nullptr, cap, block);
                    for (float v : one)
                        if (v != v) nans += cap ? 0ull : 1ull;
                        else check += v;
                }
    }
    printf("umbra driver: checksum %.9g, +inf %llu, NaN without an injected cap or a bad direction: %llu\n", check, infs, nans);
    return nans == 0ull ? 0 : 1;
}
#endif
