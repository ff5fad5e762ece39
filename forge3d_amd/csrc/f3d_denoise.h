// forge3d_amd/csrc/f3d_denoise.h -- the a-trous denoiser's arithmetic: what one lane of k_normalize and of k_atrous does for its
// pixel, how a sigma becomes a divisor, and how the tap spacing runs from pass to pass.  Host and device: tests/denoise_host
// runs these bodies on the CPU (and, stand-alone, under the address and undefined-behaviour sanitizers); f3d_denoise.hip's
// kernels are thin callers.  The operation itself is stated in f3d_denoise.hip's header and in DESIGN.md 9.2.
//
// All arithmetic is f32 in the written order, one rounding per operation (-ffp-contract=off).  expf / acosf are the platform's
// (ocml on the device, libm on the host), so host and device agree to a few ulp, not bit for bit.
//
// NON-FINITE VALUES follow NumPy's `clip` and `maximum`, which keep a NaN (the C fminf / fmaxf return the other operand):
//   * the clamp of n.n' to [-1, 1] is two comparisons, which a NaN fails: a NaN normal gives a NaN weight and, through the
//     normaliser, a NaN pixel -- it is NOT read as a normal facing the other way;
//   * max(|v|, 1e-8) of the normalisation and max(sum w, 1e-8) of the division stay fmaxf: a NaN length leaves a NaN
//     component, so every dot product with that normal is NaN whatever the other two components became; and a NaN weight
//     at a tap outside the image needs a NaN guide, normal or depth at the CENTRE (outside taps read 0), which makes the
//     centre's own tap -- inside, so in the numerator -- NaN as well: NaN / 1e-8 is the NaN that NaN / NaN would be.
#pragma once

#include <stddef.h>

#include "f3d_math.h"

namespace f3d {

struct AtrousParams {
    const float *src;     // rgb, the iterate
    float *dst;           // rgb
    const float *guide;   // rgb: albedo, or the ORIGINAL colour
    const float *normal;  // rgb, unit length (null: no normal term)
    const float *depth;   // (null: no depth term)
    uint32_t width, height;
    int step;
    uint32_t extra_albedo;  // apply the second, sigma_albedo term on the same guide difference
    float den_color, den_albedo, den_normal, den_depth;
};

// The tap spacing doubles from pass to pass and stays at 2^28 once it is there: with a spacing of max(width, height) or more
// every tap but the centre lies outside the image, so all such passes are one operation (images have sides below 2^28), and
// x + 2 * spacing stays an int for every x a pixel can have.
constexpr int kAtrousMaxStep = 1 << 28;

F3D_HD int atrous_passes(int iterations) { return iterations > 1 ? iterations : 1; }
F3D_HD int atrous_next_step(int step) { return step < kAtrousMaxStep ? step * 2 : kAtrousMaxStep; }

// np.float32(2.0 * sigma ** 2 + 1e-8): the divisor is formed in double and rounded once
F3D_HD float atrous_divisor(float sigma) { return (float)(2.0 * (double)sigma * (double)sigma + 1e-8); }

// what every pass of a call shares: the guides (normal: already normalised), the size, the divisors
F3D_HD AtrousParams atrous_params(const float *guide, const float *normal, const float *depth, uint32_t width, uint32_t height, bool albedo_given,
                                  float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth) {
    AtrousParams P{};
    P.guide = guide;
    P.normal = normal;
    P.depth = depth;
    P.width = width;
    P.height = height;
    P.extra_albedo = (albedo_given && sigma_albedo > 0.0f) ? 1u : 0u;
    P.den_color = atrous_divisor(sigma_color);
    P.den_albedo = atrous_divisor(sigma_albedo);
    P.den_normal = atrous_divisor(sigma_normal);
    P.den_depth = atrous_divisor(sigma_depth);
    return P;
}

// np.clip(c, -1, 1): a NaN stays a NaN
F3D_HD float atrous_clip_cos(float c) { return c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c); }

// normal i of `in`, v / max(1e-8, |v|), into `out`
F3D_HD void atrous_normalize(const float *in, float *out, size_t i) {
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    const float len = fmaxf(1e-8f, sqrtf(x * x + y * y + z * z));  // denoise.py:12-15
    out[3 * i] = x / len;
    out[3 * i + 1] = y / len;
    out[3 * i + 2] = z / len;
}

// pixel (x, y) of one pass: P.src -> P.dst at spacing P.step (x < width, y < height)
F3D_HD void atrous_pixel(const AtrousParams &P, int x, int y) {
    const size_t c = (size_t)y * P.width + x;
    const float g0 = P.guide[3 * c], g1 = P.guide[3 * c + 1], g2 = P.guide[3 * c + 2];
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, d0 = 0.0f;
    if (P.normal) {
        n0 = P.normal[3 * c];
        n1 = P.normal[3 * c + 1];
        n2 = P.normal[3 * c + 2];
    }
    if (P.depth) d0 = P.depth[c];
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, wsum = 0.0f;
    const float taps[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int sx = x + dx * P.step, sy = y + dy * P.step;
            const bool inside = sx >= 0 && sy >= 0 && sx < (int)P.width && sy < (int)P.height;
            const size_t s = inside ? (size_t)sy * P.width + sx : c;
            float w = taps[dy + 2] * taps[dx + 2];
            // zero padding: a tap outside the image sees guide = 0, normal = 0, depth = 0, colour = 0
            const float e0 = (inside ? P.guide[3 * s] : 0.0f) - g0, e1 = (inside ? P.guide[3 * s + 1] : 0.0f) - g1,
                        e2 = (inside ? P.guide[3 * s + 2] : 0.0f) - g2;
            const float gg = (e0 * e0 + e1 * e1) + e2 * e2;  // np.sum over the last axis: sequential
            w *= expf(-gg / P.den_color);
            if (P.extra_albedo) w *= expf(-gg / P.den_albedo);
            if (P.normal) {
                const float m0 = inside ? P.normal[3 * s] : 0.0f, m1 = inside ? P.normal[3 * s + 1] : 0.0f,
                            m2 = inside ? P.normal[3 * s + 2] : 0.0f;
                const float cosang = atrous_clip_cos((m0 * n0 + m1 * n1) + m2 * n2);
                const float ang = acosf(cosang);
                w *= expf(-(ang * ang) / P.den_normal);
            }
            if (P.depth) {
                const float dd = (inside ? P.depth[s] : 0.0f) - d0;
                w *= expf(-(dd * dd) / P.den_depth);
            }
            if (inside) {
                acc0 += P.src[3 * s] * w;
                acc1 += P.src[3 * s + 1] * w;
                acc2 += P.src[3 * s + 2] * w;
            }
            wsum += w;
        }
    }
    const float inv = fmaxf(wsum, 1e-8f);
    P.dst[3 * c] = acc0 / inv;
    P.dst[3 * c + 1] = acc1 / inv;
    P.dst[3 * c + 2] = acc2 / inv;
}

}  // namespace f3d
