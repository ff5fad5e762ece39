// tests/horizon_host/horizon_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_horizon_host.py compiles it).
// The horizon rasters' lane body (f3d_horizon.h horizon_lane, what k_horizon calls per lane) on the host over the waves and
// lanes k_horizon is launched with (f3d_walk.h region_waves / region_sample, both footprints).  The walk has no wave
// primitive in it, so a wave is a plain loop over its lanes.  `cap` (0: horizon_step_cap) injects a tiny step cap -- here
// only, the library has no such switch.
// With -DHORIZON_DRIVER the file is a stand-alone program (its own main) over a synthetic DEM, for a sanitizer build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../emul/direct_levels.h"
#include "../../forge3d_amd/csrc/f3d_horizon.h"

namespace {
void run_horizon(const TerrainDev &T, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, float lift, uint32_t count,
                 const float *azimuths, float *horizon, float *sky_view, float *origins, uint32_t cap, uint32_t block) {
    HorizonParams R{};
    R.terrain = T;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.row0 = row0;
    R.col0 = col0;
    R.rows = rows;
    R.cols = cols;
    R.lift = lift;
    R.azimuth_count = count;
    R.step_cap = cap ? cap : horizon_step_cap(T);
    R.block = block;
    R.azimuths = (const float2 *)azimuths;
    R.horizon = horizon;
    R.sky_view = sky_view;
    const long waves = region_waves(rows, cols, block);
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++)
        for (uint32_t lane = 0, n, i, j; lane < 64u; lane++)
            if (region_sample(rows, cols, block, (uint32_t)wv, lane, n)) {
                horizon_lane(R, n, DirectLevels{});
                store_point(origins, n, horizon_origin(R, n, i, j));
            }
}
}  // namespace

// info[0..5]: scene_create's first six (tests/emul/host_scene.h)
extern "C" void *horizon_scene_create(const f3d_terrain_ref_desc *d, float *info) { return scene_create(d, 1, info, 6u); }
extern "C" void horizon_scene_destroy(void *scene) { delete (HostScene *)scene; }

// How often region_sample hands out each sample over region_waves x 64 lanes: counts (rows * cols words, zeroed by the
// caller) per sample of the region; returns the samples handed out that lie outside it.
extern "C" uint32_t horizon_region_counts(uint32_t rows, uint32_t cols, uint32_t block, uint32_t *counts) {
    uint32_t outside = 0u;
    for (uint32_t wv = 0; wv < region_waves(rows, cols, block); wv++)
        for (uint32_t lane = 0, n; lane < 64u; lane++)
            if (region_sample(rows, cols, block, wv, lane, n)) {
                if (n < rows * cols) counts[n]++;
                else outside++;
            }
    return outside;
}

// One horizon raster as f3d_session_horizon's device form answers it (flags: 2 CURVED).  horizon (count x rows * cols),
// sky_view (rows * cols) and origins (rows * cols x 3: the lifted lattice points) may each be null.
extern "C" int horizon_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, float lift, uint32_t count,
                           const float *azimuths, float *horizon, float *sky_view, float *origins, uint32_t cap, uint32_t block) {
    if ((uintptr_t)azimuths % alignof(float2) != 0u) return 2;  // (read as float2: a NumPy allocation is aligned, an odd view is not)
    run_horizon(((const HostScene *)scene)->P.terrain, flags, row0, col0, rows, cols, lift, count, azimuths, horizon, sky_view, origins, cap, block);
    return 0;
}

extern "C" uint32_t horizon_step_cap_of(void *scene) { return horizon_step_cap(((const HostScene *)scene)->P.terrain); }
extern "C" uint32_t horizon_desc_size() { return (uint32_t)sizeof(f3d_session_horizon_desc); }

#if defined(HORIZON_DRIVER)
// A 65 x 63 and a 5 x 3 synthetic DEM, 16 compass azimuths and three odd ones, curved and flat, lifts 0 and 0.5, both
// footprints, a region, a tiny cap: every path of the lane body.  Prints one checksum line; exit status 0.
int main() {
    double check = 0.0;
    unsigned long long nans = 0ull;
    const uint32_t shapes[2][2] = {{65u, 63u}, {5u, 3u}};
    for (const auto &shape : shapes) {
        const uint32_t w = shape[0], h = shape[1];
        HostTables t;
        TerrainDev T{};
        driver_terrain(w, h, t, T);
        std::vector<float> az;
        for (int k = 0; k < 16; k++) {
            const double a = 6.283185307179586 * k / 16.0;
            az.push_back((float)std::sin(a));
            az.push_back((float)-std::cos(a));
        }
        const float odd[6] = {3.0f, -1.5f, -0.7f, 2.2f, 0.0f, -4.0f};
        az.insert(az.end(), odd, odd + 6);
        const uint32_t count = (uint32_t)az.size() / 2u;
        for (uint32_t flags : {0u, 2u})
            for (float lift : {0.0f, 0.5f})
                for (uint32_t block : {0u, 1u})
                    for (uint32_t cap : {0u, 3u}) {
                        const uint32_t row0 = block ? 1u : 0u, col0 = block ? 2u : 0u, rows = h - row0, cols = w - col0;
                        std::vector<float> planes((size_t)count * rows * cols), sky((size_t)rows * cols), origins((size_t)rows * cols * 3u);
                        run_horizon(T, flags, row0, col0, rows, cols, lift, count, az.data(), planes.data(), sky.data(), origins.data(), cap, block);
                        for (float v : planes) {
                            if (v != v) nans += cap ? 0ull : 1ull;
                            else if (std::isfinite(v)) check += v;
                        }
                        for (float v : sky) check += v;
                    }
    }
    printf("horizon driver: checksum %.9g, NaN without an injected cap: %llu\n", check, nans);
    return nans == 0ull ? 0 : 1;
}
#endif
