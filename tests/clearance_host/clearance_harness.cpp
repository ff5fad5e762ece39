// tests/clearance_host/clearance_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_clearance_host.py compiles it).
// The clearance rasters' lane body (f3d_clearance.h clearance_sample / clearance_height / clearance_walk, what k_clearance
// runs per lane) on the host over whole 64-lane waves, with k_clearance's two footprints: wave b owns samples
// [64 b, 64 b + 64) of the region, or an 8 x 8 block of it.  The walk has no wave primitive in it, so a wave is a plain loop
// over its lanes; the loop over the observers and the minimum are written as the kernel writes them.  `cap`
// (0: clearance_step_cap) injects a tiny step cap -- here only, the library has no such switch.
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
            const V3 g = clearance_sample(R, n, i, j);
            if (samples) {
                samples[3u * (size_t)n] = g.x;
                samples[3u * (size_t)n + 1u] = g.y;
                samples[3u * (size_t)n + 2u] = g.z;
            }
            float low = __builtin_inff();
            for (uint32_t k = 0u; k < count; k++) {
                const float4 observer{observers[4u * k], observers[4u * k + 1u], observers[4u * k + 2u], observers[4u * k + 3u]};
                const float L = clearance_height(R, g, i, j, observer, levels);
                if (height) height[(size_t)k * total + n] = L;
                low = f_min(low, L);
            }
            if (lowest) lowest[n] = low;
        }
}
}  // namespace

// info[0..5] = terrain origin x, origin z, spacing x, spacing z, inv_two_r_prime, curvature_enabled
extern "C" void *clearance_scene_create(const f3d_terrain_ref_desc *d, float *info) {
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

extern "C" void clearance_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One clearance raster as f3d_session_clearance's device form answers it (flags: 2 CURVED).  height (count x rows * cols),
// lowest (rows * cols) and samples (rows * cols x 3: the lattice points) may each be null.
extern "C" int clearance_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint32_t count,
                             const float *observers, float *height, float *lowest, float *samples, uint32_t cap, uint32_t block) {
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
        const float x_mid = plane_at(T.origin_x, w / 2u, T.spacing_x), z_last = plane_at(T.origin_z, h - 1u, T.spacing_z);
        const float z_row = plane_at(T.origin_z, h / 2u, T.spacing_z);
        const float nan = f_from_bits(0x7FC00000u);
        const float observers[] = {
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
