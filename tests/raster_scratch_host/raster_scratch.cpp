// The layout arithmetic of the rasters' host-form scratch (csrc/f3d_raster_scratch.h, which includes no HIP type) over a
// table of cases: the four families' segment lists as csrc/f3d_host_rasters.h gives them, every subset of a family's outputs,
// n samples, K inputs, and the raster without an input (SESSION_SUN).  One line a case:
//   family n K subset sun | offset of every segment in list order | total
// tests/test_raster_scratch_host.py compares them with the formulas each family carried before the lists.
#include <cstdio>

#include "../../forge3d_amd/csrc/f3d_raster_scratch.h"

static void print(const char *family, uint64_t n, uint64_t k, unsigned subset, int sun, ScratchSegment *segments, size_t count) {
    const uint64_t total = scratch_layout(segments, count);
    printf("%s %llu %llu %u %d |", family, (unsigned long long)n, (unsigned long long)k, subset, sun);
    for (size_t i = 0; i < count; i++) printf(" %llu", (unsigned long long)segments[i].offset);
    printf(" | %llu\n", (unsigned long long)total);
}

int main() {
    const uint64_t samples[] = {1u, 3u, 63u * 65u, 2049u * 2049u}, inputs[] = {0u, 1u, 3u, 16u, 256u};
    for (uint64_t n : samples)
        for (uint64_t k : inputs)
            for (unsigned subset = 0u; subset < 8u; subset++) {
                const uint64_t a = subset & 1u, b = (subset >> 1) & 1u, c = (subset >> 2) & 1u, words = (n + 63u) >> 6;
                if (subset < 4u) {
                    for (int sun = 0; sun < 2; sun++) {
                        const uint64_t targets = sun ? 1u : k;
                        ScratchSegment raster[] = {{a * targets * words * 8u, false, 0u}, {sun ? 0u : k * 16u, true, 0u}, {b * n * 4u, false, 0u}};
                        print("raster", n, k, subset, sun, raster, 3);
                    }
                    ScratchSegment horizon[] = {{a * k * n * 4u, false, 0u}, {b * n * 4u, false, 0u}, {k * 8u, true, 0u}};
                    print("horizon", n, k, subset, 0, horizon, 3);
                    ScratchSegment clearance[] = {{a * k * n * 4u, false, 0u}, {b * n * 4u, false, 0u}, {k * 16u, true, 0u}};
                    print("clearance", n, k, subset, 0, clearance, 3);
                }
                ScratchSegment irradiation[] = {{a * n * 4u, false, 0u}, {b * n * 4u, false, 0u}, {c * n * 12u, false, 0u}, {k * 16u, true, 0u}};
                print("irradiation", n, k, subset, 0, irradiation, 4);
            }
    return 0;
}
