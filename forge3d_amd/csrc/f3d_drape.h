// forge3d_amd/csrc/f3d_drape.h -- an image draped over the terrain (f3d_session_drape): per-texel albedo of terrain hits.
// What one lane does: sample the drape at a hit point (the draped frame kernels, the draped resolve) and pack one f32 texel
// into the session's binary16 buffer (k_drape_pack).  Host and device: tests/drape_host runs both bodies on the CPU.
//
// The drape is T[rows][cols] linear RGB reflectances; image row 0 lies on DEM row 0 and image column 0 on DEM column 0.
// A texel is binary16 RGBA, 8 bytes, fetched by ONE 64-bit load: x = r | g << 16, y = b | a << 16 (a is stored 0 and never
// read).  All arithmetic is f32, one rounding per written operation (the library and the emulator are compiled with
// -ffp-contract=off; nothing here spells an fma).  A terrain hit at world (x, z):
//     fx = (x - origin_x) / spacing_x              fz = (z - origin_z) / spacing_z          (DEM-sample units)
//     tx = fx * scale_x + offset_x                 tz = fz * scale_z + offset_z             (texel units: two roundings each)
//   nearest   texel clamp(floor(t + 0.5), 0, n - 1) per axis
//   bilinear  i0 = floor(t), f = t - i0, taps clamp(i0) and clamp(i0 + 1) (clamp to edge); every lerp is a + f * (b - a),
//             along x first (rows z0 and z1), then along z.  b - a is exactly 0 for equal taps, so a constant image samples
//             to exactly that constant, and so does every point whose four taps clamp to one texel.
// A NaN coordinate (it cannot come from a hit) clamps to texel 0.
#pragma once

#include "f3d_scene.h"

namespace f3d {

constexpr uint32_t kDrapeNearest = 0u, kDrapeBilinear = 1u;
constexpr float kDrapeTexelMax = 65504.0f;  // the largest finite binary16

// index of the texel a floor()ed coordinate names, clamped to [0, n - 1] (n <= 2^24).  The float is bounded by literals and
// the image size compared as an integer: no float expression of a kernel parameter is formed that the compiler could hoist
// out of the sample loop into a vector register (f3d_math.h F3D_OPAQUE_UNIFORM).
F3D_HD uint32_t drape_clamp(float floored, uint32_t n) {
    const uint32_t i = (uint32_t)f_min(f_max(floored, 0.0f), 16777216.0f);  // (f_max(NaN, 0) = 0)
    return i < n - 1u ? i : n - 1u;
}

// the value of a stored half (packed texels are finite): half_value()'s bits, on the device by the hardware's conversion --
// binary16 -> binary32 is exact for every half, subnormals included (the library keeps denormals)
F3D_HD float drape_half(uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
#else
    return half_value((uint16_t)bits);
#endif
}
F3D_HD V3 drape_texel(const DrapeDev &D, uint32_t ix, uint32_t iz) {
    const uint2 t = D.texels[(size_t)iz * D.cols + ix];
    return V3{drape_half(t.x & 0xFFFFu), drape_half(t.x >> 16), drape_half(t.y & 0xFFFFu)};
}

F3D_HD float drape_lerp(float a, float b, float f) { return a + f * (b - a); }
F3D_HD V3 drape_lerp(V3 a, V3 b, float f) { return V3{drape_lerp(a.x, b.x, f), drape_lerp(a.y, b.y, f), drape_lerp(a.z, b.z, f)}; }

// texel coordinates of world (x, z)
F3D_HD void drape_coords(const DrapeDev &D, const TerrainDev &T, float x, float z, float &tx, float &tz) {
    float sx = T.spacing_x, sz = T.spacing_z;
    // (render constants: the divisions' operands are formed per sample, not held in vector registers across the kernel; the
    // values are kernel parameters, still in scalar registers here, so the scalar form of F3D_OPAQUE_UNIFORM is accepted)
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(sx));
    asm volatile("" : "+s"(sz));
#endif
    const float fx = (x - T.origin_x) / sx, fz = (z - T.origin_z) / sz;
    tx = fx * D.scale_x + D.offset_x;
    tz = fz * D.scale_z + D.offset_z;
}

// the drape at texel coordinates (tx, tz)
F3D_HD V3 drape_sample_at(const DrapeDev &D, float tx, float tz) {
    if (D.filter == kDrapeNearest)
        return drape_texel(D, drape_clamp(f_floor(tx + 0.5f), D.cols), drape_clamp(f_floor(tz + 0.5f), D.rows));
    const float x0 = f_floor(tx), z0 = f_floor(tz);
    const float fx = tx - x0, fz = tz - z0;
    const uint32_t ix0 = drape_clamp(x0, D.cols), ix1 = drape_clamp(x0 + 1.0f, D.cols);
    const uint32_t iz0 = drape_clamp(z0, D.rows), iz1 = drape_clamp(z0 + 1.0f, D.rows);
    const V3 t00 = drape_texel(D, ix0, iz0), t10 = drape_texel(D, ix1, iz0);
    const V3 t01 = drape_texel(D, ix0, iz1), t11 = drape_texel(D, ix1, iz1);
    return drape_lerp(drape_lerp(t00, t10, fx), drape_lerp(t01, t11, fx), fz);
}

// the albedo of a terrain hit at world (x, z)
F3D_HD V3 drape_sample(const DrapeDev &D, const TerrainDev &T, float x, float z) {
    float tx, tz;
    drape_coords(D, T, x, z, tx, tz);
    return drape_sample_at(D, tx, tz);
}

// ---- packing: f32 RGB(A), row-major, into the binary16 buffer -- the whole image or a window of it -----------------------
// A value that is not a reflectance a half can hold -- non-finite, negative, above 65504 -- is stored as 0 (the host form of
// f3d_session_drape refuses such an image before anything is uploaded; the device form cannot look).
struct DrapePackParams {
    const float *src;         // rows x cols x channels f32: the window's texels
    uint2 *dst;               // the session's drape, dst_cols texels a row
    uint32_t rows, cols;      // of the window
    uint32_t channels;        // 3 or 4 (a fourth channel is ignored)
    uint32_t dst_cols;
    uint32_t at_row, at_col;  // the window's first texel in dst
};

F3D_HD uint32_t drape_pack_channel(float v) {
    const bool good = f_finite(v) && v >= 0.0f && v <= kDrapeTexelMax;
    return (uint32_t)half_bits(good ? v : 0.0f);
}
F3D_HD uint2 drape_pack_texel(float r, float g, float b) {
    return uint2{drape_pack_channel(r) | (drape_pack_channel(g) << 16), drape_pack_channel(b)};
}
// texel (r, c) of the window: r < rows, c < cols
F3D_HD void drape_pack_at(const DrapePackParams &B, uint32_t r, uint32_t c) {
    const float *s = B.src + ((size_t)r * B.cols + c) * B.channels;
    B.dst[(size_t)(B.at_row + r) * B.dst_cols + (B.at_col + c)] = drape_pack_texel(s[0], s[1], s[2]);
}

}  // namespace f3d
