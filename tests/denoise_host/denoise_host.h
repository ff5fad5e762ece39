// tests/denoise_host/denoise_host.h -- TEST INFRASTRUCTURE ONLY.  One call of the a-trous denoiser on the host: what
// f3d_atrous_denoise (csrc/f3d_denoise.hip) does with its device buffers and launches, done with vectors and loops over the
// same bodies of csrc/f3d_denoise.h -- every lane of k_normalize, then per pass every lane of k_atrous.
#pragma once

#include <cstdint>
#include <vector>

#include "../../forge3d_amd/csrc/f3d_denoise.h"

inline void denoise_host(const float *color, const float *albedo, const float *normal, const float *depth, uint32_t width, uint32_t height,
                         int32_t iterations, float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth, float *out) {
    using namespace f3d;
    const size_t px = (size_t)width * height;
    std::vector<float> a(3 * px), b(3 * px), unit(normal ? 3 * px : 0);
    for (size_t i = 0; normal && i < px; i++) atrous_normalize(normal, unit.data(), i);
    AtrousParams P = atrous_params(albedo ? albedo : color, normal ? unit.data() : nullptr, depth, width, height, albedo != nullptr, sigma_color,
                                   sigma_albedo, sigma_normal, sigma_depth);
    const int passes = atrous_passes(iterations);
    const float *src = color;
    float *dst = a.data();
    for (int i = 0, step = 1; i < passes; i++, step = atrous_next_step(step)) {
        P.src = src;
        P.dst = dst;
        P.step = step;
        for (int y = 0; y < (int)height; y++)
            for (int x = 0; x < (int)width; x++) atrous_pixel(P, x, y);
        src = dst;
        dst = dst == a.data() ? b.data() : a.data();
    }
    for (size_t i = 0; i < 3 * px; i++) out[i] = src[i];
}
