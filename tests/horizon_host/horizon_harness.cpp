// tests/horizon_host/horizon_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_horizon_host.py compiles it).
// The horizon rasters' lane body (f3d_horizon.h horizon_origin / horizon_walk / horizon_sky_term, what k_horizon runs per
// lane) on the host over whole 64-lane waves, with k_horizon's two footprints: wave b owns samples [64 b, 64 b + 64) of the
// region, or an 8 x 8 block of it.  The walk has no wave primitive in it, so a wave is a plain loop over its lanes; the loop
// over the azimuths and the sky-view sum are written as the kernel writes them.  `cap` (0: horizon_step_cap) injects a tiny
// step cap -- here only, the library has no such switch.
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
    const uint32_t total = rows * cols, tiles_x = (cols + 7u) >> 3;
    const long waves = block ? (long)tiles_x * ((rows + 7u) >> 3) : ((long)total + 63) / 64;
    const DirectLevels levels;
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t n = (uint32_t)wv * 64u + lane;
            bool have = n < total;
            if (block) {
                const uint32_t r = ((uint32_t)wv / tiles_x) * 8u + (lane >> 3), c = ((uint32_t)wv % tiles_x) * 8u + (lane & 7u);
                have = r < rows && c < cols;
                n = r * cols + c;
            }
            if (!have) continue;
            uint32_t i, j;
            const V3 o = horizon_origin(R, n, i, j);
            if (origins) {
                origins[3u * (size_t)n] = o.x;
                origins[3u * (size_t)n + 1u] = o.y;
                origins[3u * (size_t)n + 2u] = o.z;
            }
            float sum = 0.0f;
            for (uint32_t k = 0u; k < count; k++) {
                const float dx = azimuths[2u * k], dz = azimuths[2u * k + 1u];
                const float H = horizon_walk(T, o, i, j, dx, dz, horizon_curvature(R, dx, dz), R.step_cap, levels);
                if (horizon) horizon[(size_t)k * total + n] = H;
                sum = sum + horizon_sky_term(H, dx, dz);
            }
            if (sky_view) sky_view[n] = 1.0f - sum / (float)count;
        }
}
}  // namespace

// info[0..5] = terrain origin x, origin z, spacing x, spacing z, inv_two_r_prime, curvature_enabled
extern "C" void *horizon_scene_create(const f3d_terrain_ref_desc *d, float *info) {
    HostScene *S = new HostScene();
    try {
        setup(*S, d, 1, 0u, 0u);
    } catch (const Failure &) {
        delete S;
        return nullptr;
    }
    if (info) {
        info[0] = S->P.terrain.origin_x;
        info[1] = S->P.terrain.origin_z;
        info[2] = S->P.terrain.spacing_x;
        info[3] = S->P.terrain.spacing_z;
        info[4] = S->P.terrain.inv_two_r_prime;
        info[5] = (float)S->P.terrain.curvature_enabled;
    }
    return S;
}

extern "C" void horizon_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One horizon raster as f3d_session_horizon's device form answers it (flags: 2 CURVED).  horizon (count x rows * cols),
// sky_view (rows * cols) and origins (rows * cols x 3: the lifted lattice points) may each be null.
extern "C" int horizon_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, float lift, uint32_t count,
                           const float *azimuths, float *horizon, float *sky_view, float *origins, uint32_t cap, uint32_t block) {
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
        std::vector<float> dem((size_t)w * h);
        for (uint32_t z = 0; z < h; z++)
            for (uint32_t x = 0; x < w; x++) dem[(size_t)z * w + x] = 3.0f * std::sin(0.37f * (float)x) * std::cos(0.23f * (float)z) + 0.05f * (float)((x * 7u + z * 13u) % 11u);
        HostTables t = build_tables_host(dem.data(), w, h, 20.0f);
        TerrainDev T{};
        t.attach(T);
        T.spacing_x = 30.0f;
        T.spacing_z = 25.0f;
        T.inv_spacing_x = 1.0f / T.spacing_x;
        T.inv_spacing_z = 1.0f / T.spacing_z;
        T.origin_x = -0.5f * ((float)w - 1.0f) * T.spacing_x;
        T.origin_z = -0.5f * ((float)h - 1.0f) * T.spacing_z;
        T.inv_two_r_prime = 6.7e-8f;
        T.curvature_enabled = 1u;
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
