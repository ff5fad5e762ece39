// tests/clearance_host/clearance_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_clearance_host.py compiles it).
// The clearance rasters' lane body (f3d_clearance.h clearance_lane, what k_clearance calls per lane) on the host over the
// waves and lanes k_clearance is launched with (f3d_walk.h region_waves / region_sample, both footprints).  The walk has no
// wave primitive in it, so a wave is a plain loop over its lanes.  `cap` (0: clearance_step_cap) injects a tiny step cap --
// here only, the library has no such switch.
// With -DCLEARANCE_DRIVER the file is a stand-alone program (its own main) over two synthetic DEMs, for a sanitizer build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../emul/direct_levels.h"
#include "../../forge3d_amd/csrc/f3d_clearance.h"

namespace {
void run_clearance(const TerrainDev &T, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint32_t count,
                   const float *observers, float *height, float *lowest, float *samples, uint32_t cap, uint32_t block) {
    ClearanceParams R{};
    R.terrain = T;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.row0 = row0;
    R.col0 = col0;
    R.rows = rows;
    R.cols = cols;
    R.observer_count = count;
    R.step_cap = cap ? cap : clearance_step_cap(T);
    R.block = block;
    R.observers = (const float4 *)observers;
    R.height = height;
    R.lowest = lowest;
    const long waves = region_waves(rows, cols, block);
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++)
        for (uint32_t lane = 0, n, i, j; lane < 64u; lane++)
            if (region_sample(rows, cols, block, (uint32_t)wv, lane, n)) {
                clearance_lane(R, n, DirectLevels{});
                store_point(samples, n, clearance_sample(R, n, i, j));
            }
}
}  // namespace

// info[0..5]: scene_create's first six (tests/emul/host_scene.h)
extern "C" void *clearance_scene_create(const f3d_terrain_ref_desc *d, float *info) { return scene_create(d, 1, info, 6u); }
extern "C" void clearance_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One clearance raster as f3d_session_clearance's device form answers it (flags: 2 CURVED).  height (count x rows * cols),
// lowest (rows * cols) and samples (rows * cols x 3: the lattice points) may each be null.
extern "C" int clearance_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint32_t count,
                             const float *observers, float *height, float *lowest, float *samples, uint32_t cap, uint32_t block) {
    if ((uintptr_t)observers % alignof(float4) != 0u) return 2;  // (read as float4: a NumPy allocation is aligned, an odd view is not)
    run_clearance(((const HostScene *)scene)->P.terrain, flags, row0, col0, rows, cols, count, observers, height, lowest, samples, cap, block);
    return 0;
}

extern "C" uint32_t clearance_step_cap_of(void *scene) { return clearance_step_cap(((const HostScene *)scene)->P.terrain); }
extern "C" uint32_t clearance_desc_size() { return (uint32_t)sizeof(f3d_session_clearance_desc); }

#if defined(CLEARANCE_DRIVER)
// A 65 x 63 and a 5 x 3 synthetic DEM; observers over, outside, on a lattice column, on a lattice corner, on the last lattice
// line, under the surface, with a distance limit, non-finite; curved and flat, both footprints, a region, a tiny cap: every
// path of the lane body.  Prints one checksum line; exit status 0.
int main() {
    double check = 0.0;
    unsigned long long nans = 0ull, infs = 0ull;
    const uint32_t shapes[2][2] = {{65u, 63u}, {5u, 3u}};
    for (const auto &shape : shapes) {
        const uint32_t w = shape[0], h = shape[1];
        HostTables t;
        TerrainDev T{};
        driver_terrain(w, h, t, T);
        const float x_mid = plane_at(T.origin_x, w / 2u, T.spacing_x), z_last = plane_at(T.origin_z, h - 1u, T.spacing_z);
        const float z_row = plane_at(T.origin_z, h / 2u, T.spacing_z);
        const float nan = f_from_bits(0x7FC00000u);
        alignas(16) const float observers[] = {
            0.3f * T.origin_x, 150.0f, 0.2f * T.origin_z, 0.0f,    // high over the footprint
            -0.2f * T.origin_x, 120.0f, 0.1f * T.origin_z, 400.0f,  // a distance limit
            1.4f * T.origin_x, 90.0f, -0.3f * T.origin_z, 0.0f,     // outside the footprint
            x_mid, 110.0f, 0.37f * T.origin_z, 0.0f,                // on a lattice column: a column of flat-axis walks
            x_mid, 130.0f, z_row, 0.0f,                             // on a lattice corner: hd2 == 0 for one sample
            0.11f * T.origin_x, 140.0f, z_last, 0.0f,               // on the DEM's last lattice line
            0.13f * T.origin_x, -500.0f, 0.17f * T.origin_z, 0.0f,  // under the surface
            nan, 100.0f, 0.0f, 0.0f,                                // the device form's NaN plane
        };
        const uint32_t count = (uint32_t)(sizeof(observers) / sizeof(float)) / 4u;
        for (uint32_t flags : {0u, 2u})
            for (uint32_t block : {0u, 1u})
                for (uint32_t cap : {0u, 3u}) {
                    const uint32_t row0 = block ? 1u : 0u, col0 = block ? 2u : 0u, rows = h - row0, cols = w - col0;
                    std::vector<float> planes((size_t)count * rows * cols), low((size_t)rows * cols), samples((size_t)rows * cols * 3u);
                    run_clearance(T, flags, row0, col0, rows, cols, count, observers, planes.data(), low.data(), samples.data(), cap, block);
                    for (size_t q = 0; q < planes.size(); q++) {
                        const float v = planes[q];
                        if (v != v) nans += (cap || q / ((size_t)rows * cols) == count - 1u) ? 0ull : 1ull;
                        else if (std::isfinite(v)) check += v;
                        else infs++;
                    }
                    for (float v : low)
                        if (std::isfinite(v)) check += v;
                }
    }
    printf("clearance driver: checksum %.9g, +inf %llu, NaN without an injected cap or a NaN observer: %llu\n", check, infs, nans);
    return nans == 0ull ? 0 : 1;
}
#endif
