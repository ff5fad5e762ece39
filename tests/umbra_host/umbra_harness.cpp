// tests/umbra_host/umbra_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_umbra_host.py compiles it).
// The shadow-depth rasters' lane body (f3d_umbra.h umbra_sample / umbra_depth / umbra_walk, what k_umbra runs per lane) on the
// host over whole 64-lane waves, with k_umbra's two footprints: wave b owns samples [64 b, 64 b + 64) of the region, or an
// 8 x 8 block of it.  The walk has no wave primitive in it, so a wave is a plain loop over its lanes; the loop over the
// directions and the maximum are written as the kernel writes them.  `cap` (0: horizon_step_cap) injects a tiny step cap --
// here only, the library has no such switch.  umbra_horizon_run is the horizon raster's lane body (f3d_horizon.h) over the
// same scene, for the cross-check of the two walks.
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
            const V3 g = umbra_sample(R, n, i, j);
            if (samples) {
                samples[3u * (size_t)n] = g.x;
                samples[3u * (size_t)n + 1u] = g.y;
                samples[3u * (size_t)n + 2u] = g.z;
            }
            float deep = 0.0f;
            for (uint32_t k = 0u; k < count; k++) {
                const float4 direction = directions ? float4{directions[4u * k], directions[4u * k + 1u], directions[4u * k + 2u], directions[4u * k + 3u]}
                                                    : float4{R.sun.x, R.sun.y, R.sun.z, 0.0f};
                const float L = umbra_depth(R, g, i, j, direction, levels);
                if (depth) depth[(size_t)k * total + n] = L;
                deep = f_max(deep, L);
            }
            if (deepest) deepest[n] = deep;
        }
}
}  // namespace

// info[0..8] = terrain origin x, origin z, spacing x, spacing z, inv_two_r_prime, curvature_enabled, the sun direction
extern "C" void *umbra_scene_create(const f3d_terrain_ref_desc *d, float *info) {
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
        info[6] = S->P.light.wi.x;
        info[7] = S->P.light.wi.y;
        info[8] = S->P.light.wi.z;
    }
    return S;
}

extern "C" void umbra_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One shadow-depth raster as f3d_session_umbra's device form answers it (flags: 2 CURVED, 16 SESSION_SUN: directions null, count 1).
// depth (count x rows * cols), deepest (rows * cols) and samples (rows * cols x 3: the lattice points) may each be null.
extern "C" int umbra_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint32_t count,
                         const float *directions, float *depth, float *deepest, float *samples, uint32_t cap, uint32_t block) {
    const HostScene *S = (const HostScene *)scene;
    const bool sun = (flags & 16u) != 0u;
    if (sun != (directions == nullptr) || (sun && count != 1u)) return 1;
    run_umbra(S->P.terrain, S->P.light.wi, flags, row0, col0, rows, cols, count, directions, depth, deepest, samples, cap, block);
    return 0;
}

// The horizon raster's lane body at `lift` over the whole DEM: horizon (count x rows * cols) for azimuths (count x 2).
extern "C" int umbra_horizon_run(void *scene, uint32_t flags, float lift, uint32_t count, const float *azimuths, float *horizon) {
    const TerrainDev &T = ((const HostScene *)scene)->P.terrain;
    HorizonParams R{};
    R.terrain = T;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.rows = T.cell_h + 1u;
    R.cols = T.cell_w + 1u;
    R.lift = lift;
    R.azimuth_count = count;
    R.step_cap = horizon_step_cap(T);
    const uint32_t total = R.rows * R.cols;
    const DirectLevels levels;
#pragma omp parallel for schedule(dynamic, 64)
    for (long n = 0; n < (long)total; n++) {
        uint32_t i, j;
        const V3 o = horizon_origin(R, (uint32_t)n, i, j);
        for (uint32_t k = 0u; k < count; k++) {
            const float dx = azimuths[2u * k], dz = azimuths[2u * k + 1u];
            horizon[(size_t)k * total + (size_t)n] = horizon_walk(T, o, i, j, dx, dz, horizon_curvature(R, dx, dz), R.step_cap, levels);
        }
    }
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
        const float nan = f_from_bits(0x7FC00000u);
        const float directions[] = {
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
