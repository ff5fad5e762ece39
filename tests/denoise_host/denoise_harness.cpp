// tests/denoise_host/denoise_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_denoise_host.py compiles it).
// The bodies of csrc/f3d_denoise.h on the host: a whole call (denoise_host.h), and the pass loop's tap spacings.
#include "denoise_host.h"

// null pointers for the guides that are not given; out: height x width x 3
extern "C" void denoise_run(const float *color, const float *albedo, const float *normal, const float *depth, uint32_t width, uint32_t height,
                            int32_t iterations, float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth, float *out) {
    denoise_host(color, albedo, normal, depth, width, height, iterations, sigma_color, sigma_albedo, sigma_normal, sigma_depth, out);
}

// the spacing of every pass of a call with `iterations`, into steps[capacity]; returns the number of passes
extern "C" int32_t denoise_steps(int32_t iterations, int32_t *steps, int32_t capacity) {
    const int passes = f3d::atrous_passes(iterations);
    for (int i = 0, step = 1; i < passes; i++, step = f3d::atrous_next_step(step))
        if (i < capacity) steps[i] = step;
    return passes;
}

extern "C" float denoise_divisor(float sigma) { return f3d::atrous_divisor(sigma); }
