// tests/denoise_host/denoise_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program over the bodies of csrc/f3d_denoise.h,
// for tests/test_denoise_host.py to compile with -fsanitize=address,undefined -fno-sanitize-recover=all and run: every read
// behind a buffer and every signed overflow of the tap arithmetic ends it with a report and a non-zero status.
//
//     denoise_main HEIGHT WIDTH ITERATIONS
//
// All guides, buffers of exactly the image's size on the heap (so one texel too far is a report), one NaN normal and one Inf
// depth among the inputs.  Prints the number of non-finite values and the sum of the finite ones.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "denoise_host.h"

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s HEIGHT WIDTH ITERATIONS\n", argv[0]);
        return 2;
    }
    const uint32_t h = (uint32_t)atoi(argv[1]), w = (uint32_t)atoi(argv[2]);
    const int iterations = atoi(argv[3]);
    const size_t px = (size_t)w * h;
    if (px == 0) return 2;
    std::vector<float> color(3 * px), albedo(3 * px), normal(3 * px), depth(px), out(3 * px);
    uint32_t state = 20261020u;
    auto uniform = [&]() {
        state = state * 1664525u + 1013904223u;
        return (float)(state >> 8) / 16777216.0f;
    };
    for (size_t i = 0; i < px; i++) {
        for (int k = 0; k < 3; k++) {
            color[3 * i + k] = uniform();
            albedo[3 * i + k] = 0.25f + 0.5f * (float)((i / 3 + k) % 2);
            normal[3 * i + k] = uniform() - 0.3f;
        }
        depth[i] = 10.0f + uniform();
    }
    normal[3 * (px / 2) + 1] = NAN;
    depth[px - 1] = INFINITY;
    denoise_host(color.data(), albedo.data(), normal.data(), depth.data(), w, h, iterations, 0.1f, 0.2f, 0.3f, 0.5f, out.data());
    size_t bad = 0;
    double sum = 0.0;
    for (float v : out) {
        if (std::isfinite(v)) sum += v;
        else bad++;
    }
    printf("%ux%u, %d iterations: %zu non-finite, sum %.9g\n", h, w, iterations, bad, sum);
    return 0;
}
