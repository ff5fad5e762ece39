// tests/irradiation_host/irradiation_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_irradiation_host.py compiles it).
// The irradiation rasters' lane body (f3d_irradiation.h irradiation_origin / irradiation_slope / irradiation_term /
// irradiation_normal, what k_irradiation runs per lane) on the host over whole 64-lane waves: wave b owns samples
// [64 b, 64 b + 64) of the region, as on the device.  The lanes are the emulator's fibers and the marches' votes are exchanged
// in lockstep; a wave is run once per direction, and a lane whose term is settled without a ray (a facet turned away, a weight
// that is not positive, a refused direction) leaves that wave without having voted -- the region k_irradiation's lanes skip
// with their EXEC bit off.  The sum and the count are kept per lane across the directions as the kernel keeps them.
// The loop over the directions below is this harness's own, NOT k_irradiation's: here every direction gets a fresh pending
// context and a wave of its own; on the device one context and its LDS rows serve all directions.  That loop is covered by
// tests/test_gpu_irradiation.py; what runs here is the lane body.
// With -DIRRADIATION_DRIVER the file is a stand-alone program (its own main) over a synthetic DEM, for a sanitizer build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../../forge3d_amd/csrc/f3d_irradiation.h"

namespace {
struct IrradiationPending : WavePending {
    static constexpr bool kShareClosest = false;
};

// flags: 1 TERRAIN_ONLY, 2 CURVED, 16 HORIZONTAL.  Every output may be null.
void run_irradiation(const FrameParams &P, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, float lift, uint32_t count,
                     const float *directions, float *energy, uint32_t *seen_out, float *normal, uint32_t *marches, float *origins) {
    IrradiationParams R{};
    R.frame = P;
    if (flags & 1u) R.frame.mesh.traversal_mode = 3u;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.horizontal = (flags & 16u) ? 1u : 0u;
    R.row0 = row0;
    R.col0 = col0;
    R.rows = rows;
    R.cols = cols;
    R.lift = lift;
    R.direction_count = count;
    R.directions = (const float4 *)directions;
    const uint32_t total = rows * cols;
    const long waves = ((long)total + 63) / 64;
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++) {
        Wave wave;
        const uint32_t first = (uint32_t)wv * 64u, n = total - first < 64u ? total - first : 64u;
        const uint64_t lanes = n == 64u ? ~0ull : ((1ull << n) - 1ull);
        V3 o[64];
        IrradiationSlope s[64];
        float sum[64] = {};
        uint32_t seen[64] = {};
        for (uint32_t l = 0; l < n; l++) {
            uint32_t i, j;
            o[l] = irradiation_origin(R, first + l, i, j);
            s[l] = irradiation_slope(R, i, j);
            store_point(origins, first + l, o[l]);
        }
        for (uint32_t k = 0; k < count; k++) {
            const float4 dir = R.directions[k];
            wave.run(lanes, [&](int lane) {
                IrradiationPending pend;
                pend.wave = &wave;
                pend.me = lane;
                std::vector<RayLog> log;
                pend.log = &log;
                bool lit = false;
                const float term = irradiation_term(R, o[lane], s[lane], dir, pend, lit);
                if (lit) {  // (fibers of one thread: no race)
                    sum[lane] = sum[lane] + term;
                    seen[lane] += 1u;
                }
                if (marches) marches[(size_t)k * total + first + (uint32_t)lane] = (uint32_t)log.size();
            });
        }
        for (uint32_t l = 0; l < n; l++) {
            if (energy) energy[first + l] = sum[l];
            if (seen_out) seen_out[first + l] = seen[l];
            store_point(normal, first + l, irradiation_normal(s[l]));
        }
    }
}
}  // namespace

// One irradiation raster as f3d_session_irradiation's device form answers it, over a scene made by the raster harness's
// raster_scene_create (tests/raster_host: the same HostScene).  marches (count x rows * cols words, may be null): how many
// terrain marches the lane of sample n entered for direction k.
extern "C" void *irradiation_scene_create(const f3d_terrain_ref_desc *d, int32_t mesh_form, float *info) { return scene_create(d, mesh_form, info, 9u); }
extern "C" void irradiation_scene_destroy(void *scene) { delete (HostScene *)scene; }

extern "C" int irradiation_run(void *scene, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, float lift, uint32_t count,
                               const float *directions, float *energy, uint32_t *seen, float *normal, uint32_t *marches, float *origins) {
    run_irradiation(((const HostScene *)scene)->P, flags, row0, col0, rows, cols, lift, count, directions, energy, seen, normal, marches, origins);
    return 0;
}

extern "C" uint32_t irradiation_desc_size() { return (uint32_t)sizeof(f3d_session_irradiation_desc); }

#if defined(IRRADIATION_DRIVER)
// A 65 x 63 and a 5 x 3 synthetic DEM, terrain only; ten directions -- a day's arc, one below the horizontal, a zero weight, a
// zero direction, a NaN component --, curved and flat, HORIZONTAL and not, a region: every path of the lane body.  Prints one
// checksum line; exit status 0 when the terms that must not march did not.
int main() {
    double check = 0.0;
    unsigned long long bad = 0ull, marched = 0ull, lit = 0ull;
    const uint32_t shapes[2][2] = {{65u, 63u}, {5u, 3u}};
    for (const auto &shape : shapes) {
        const uint32_t w = shape[0], h = shape[1];
        HostTables t;
        FrameParams P{};
        driver_terrain(w, h, t, P.terrain);
        P.mesh.traversal_mode = 3u;
        std::vector<float> dirs;
        for (int k = 0; k < 6; k++) {
            const double az = 1.5707963267948966 + 3.141592653589793 * (k + 0.5) / 6.0, el = 0.06 + 0.8 * std::sin(3.141592653589793 * (k + 0.5) / 6.0);
            const float row[4] = {(float)(std::sin(az) * std::cos(el)), (float)std::sin(el), (float)(-std::cos(az) * std::cos(el)), 100.0f + 50.0f * (float)k};
            dirs.insert(dirs.end(), row, row + 4);
        }
        const float odd[16] = {0.5f, -0.2f, 0.5f, 1.0f, 0.3f, 0.4f, 0.1f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.3f, std::nanf(""), 0.1f, 1.0f};
        dirs.insert(dirs.end(), odd, odd + 16);
        const uint32_t count = (uint32_t)dirs.size() / 4u;
        for (uint32_t flags : {1u, 3u, 17u, 19u})
            for (uint32_t window : {0u, 1u}) {
                const uint32_t row0 = window ? 1u : 0u, col0 = window ? 2u : 0u, rows = h - row0, cols = w - col0;
                const size_t n = (size_t)rows * cols;
                std::vector<float> energy(n), normal(3u * n), origins(3u * n);
                std::vector<uint32_t> seen(n), marches((size_t)count * n);
                run_irradiation(P, flags, row0, col0, rows, cols, 1e-3f, count, dirs.data(), energy.data(), seen.data(), normal.data(), marches.data(),
                                origins.data());
                for (size_t i = 0; i < n; i++) {
                    check += energy[i] + normal[3u * i] + normal[3u * i + 1u] + normal[3u * i + 2u];
                    lit += seen[i];
                    if (!std::isfinite(energy[i]) || energy[i] < 0.0f || seen[i] > 7u) bad++;  // (the arc and, on a steep facet, the one below the horizontal)
                    for (uint32_t k = 0; k < count; k++) {
                        marched += marches[(size_t)k * n + i];
                        if (k >= 7u && marches[(size_t)k * n + i] != 0u) bad++;  // (zero weight, zero direction, NaN: never marched)
                    }
                }
            }
    }
    printf("irradiation driver: checksum %.9g, %llu marches, %llu terms lit, terms that broke the contract: %llu\n", check, marched, lit, bad);
    return bad == 0ull && lit != 0ull ? 0 : 1;
}
#endif
