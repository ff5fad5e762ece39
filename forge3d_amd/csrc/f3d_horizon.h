// forge3d_amd/csrc/f3d_horizon.h -- horizon rasters on a live session (f3d_session_horizon): what one lane of k_horizon does.
//
// THE CONTRACT.  Terrain only: a session with a mesh answers for the ground.  Sample n of the region is DEM sample (j, i) and
// stands on o = (x_i, h(i, j) + lift, z_j), the visibility rasters' lifted lattice point (lattice_point, f3d_walk.h; lift >= 0).
// An azimuth is a horizontal direction (dx, dz), f32, used as given.  With p(t) = (o.x + t dx, o.z + t dz) and y(p) the
// bilinear surface of the cell under p (the leaf record's four corners), the horizon of the sample along the azimuth is
//     H = sup over t > 0 with p(t) inside the DEM's footprint of ( y(p(t)) - k t^2 - o.y ) / t
// where k = (dx^2 + dz^2) inv_two_r_prime under the curvature policy (CURVED on a scene whose curvature is enabled: make_ray's
// c2) and 0 otherwise -- the drop the curved march adds to a ray's height (f3d_trace.h height_at), so (dx, H, dz) is the
// grazing direction of occluded() for the same flag.  H is a rise per unit parameter: for a unit (dx, dz) the tangent of the
// horizon's elevation.  No terrain along the azimuth (a border sample looking outward): H = -inf.  With lift == 0 the
// supremum includes the limit t -> 0+, the surface's directional derivative.
// The footprint, the lattice, the treatment of a zero component and why there is no tie bookkeeping: f3d_walk.h.  Along the
// last lattice line of an axis -- the far border edge -- the line meets no cell and H = -inf.
//
// THE LEAF.  Inside one cell the line spends [t0, t1] and y(p(t)) - o.y - k t^2 is the quadratic A t^2 + B t + C of SampleRay
// (f3d_walk.h), counted from the sample: in the sample's own cell C = hb - o.y is -lift to the bit (0 with lift == 0: the
// limit t -> 0+ is B, with no 0 / 0).
// The supremum of g(t) = A t + B + C / t over the segment is at t0, at t1, or at t* = sqrt(C / A) when t* lies strictly
// inside (a maximum exactly when A < 0 and C < 0; g(t*) = 2 A t* + B).  g(t0) is evaluated in the first cell only (t0 = 0):
// every later t0 is a point the previous cell, or a skipped node whose bound covers it, has already answered for.
//
// THE WALK is pyramid_walk (f3d_walk.h) as a ray from the sample, with empty() = -inf.  THE NODE BOUND is slope_may_raise's
// with n = mx - o.y.  best only grows, so terrain behind a crest and below the eye is rejected at coarse levels; on rising
// ground every cell up to the crest can raise the horizon and is evaluated (a band maximum cannot reject a node whose far end
// is much farther than its near end).  A walk that exceeds the step cap (walk_step_cap): that azimuth of that sample is qNaN.
//
// All arithmetic is f32, one rounding per written operation (f3d_math.h), so the host build (tests/horizon_host) and the
// device return the same bits.  sky_view is the horizontal-surface sky-view factor of Dozier-Frew / Zaksek,
//     1 - (sum_k s_k) / K,   s_k = max(h, 0) / sqrt(1 + h^2),  h = H_k / sqrt(dx_k^2 + dz_k^2)
// (s_k: the sine of the horizon's elevation), summed for k = 0 .. K - 1 in f32 with every operation rounded on its own -- no
// fma, so that NumPy reproduces it from the planes bit for bit; -inf and NaN azimuths contribute 0.
#pragma once

#include "f3d_walk.h"

namespace f3d {

constexpr uint32_t kHorizonMaxAzimuths = 256u;

// the step cap of the horizon and shadow-depth walks: the walk's (the name the host path and the harnesses call)
F3D_HD uint32_t horizon_step_cap(const TerrainDev &T) { return walk_step_cap(T); }

// DEM sample (i, j) of sample n of the region, and its lifted lattice point
F3D_HD V3 horizon_origin(const HorizonParams &R, uint32_t n, uint32_t &i, uint32_t &j) {
    return lattice_point(R.terrain, R.row0, R.col0, R.cols, n, R.lift, i, j);
}

// The curvature coefficient of an azimuth: make_ray's c2.
F3D_HD float horizon_curvature(const HorizonParams &R, float dx, float dz) {
    const bool curved = R.curved != 0u && R.terrain.curvature_enabled != 0u;
    return curved ? dot2(dx, dz, dx, dz) * R.terrain.inv_two_r_prime : 0.0f;
}

// What the sample's sky-view sum takes from one azimuth (see the header: no fma).
F3D_HD float horizon_sky_term(float H, float dx, float dz) {
    const float h = H / f_sqrt(dx * dx + dz * dz);
    return h > 0.0f ? h / f_sqrt(1.0f + h * h) : 0.0f;  // (-inf, NaN: 0)
}

// The horizon's policy of pyramid_walk (f3d_walk.h): the header's node bound, and the header's leaf.
struct HorizonPolicy : SampleRay {
    using SampleRay::SampleRay;
    static F3D_HD float empty() { return -__builtin_inff(); }
    F3D_HD bool may_raise(float mx, float t0, float t1, float best) const { return slope_may_raise(mx - oy, k, t0, t1, best); }
    F3D_HD bool leaf(const TerrainDev &T, uint32_t nx, uint32_t nz, float t0, float t1, float t_start, float &best) const {
        float A, B, C;
        quadratic(T, nx, nz, A, B, C);
        if (!(t0 > t_start)) best = f_max(best, C < 0.0f ? -__builtin_inff() : B);  // the sample's own cell: the limit t -> 0+
        if (t1 > t0) {
            best = f_max(best, f_fma(A, t1, B) + C / t1);
            if (A < 0.0f && C < 0.0f) {
                const float ts = f_sqrt(C / A);
                if (ts > t0 && ts < t1) best = f_max(best, f_fma(2.0f * A, ts, B));
            }
        }
        return false;
    }
};

// One lane, one azimuth: the horizon of the sample (i, j) standing on o along (dx, dz).  Levels: see pyramid_walk.
template <class Levels>
F3D_HD float horizon_walk(const TerrainDev &T, V3 o, uint32_t i, uint32_t j, float dx, float dz, float k, uint32_t cap, const Levels &levels) {
    if (!(f_finite(dx) && f_finite(dz)) || (dx == 0.0f && dz == 0.0f)) return f_from_bits(0x7FC00000u);
    return pyramid_walk(T, o.x, o.z, dx, dz, i, j, cap, levels, HorizonPolicy(T, o.y, i, j, dx, dz, k));
}

// One lane, sample n of the region (what k_horizon calls): every azimuth's plane, and the sky view.  No wave primitive.
template <class Levels>
F3D_HD void horizon_lane(const HorizonParams R, uint32_t n, const Levels &levels) {
    const uint32_t total = R.rows * R.cols;
    uint32_t i, j;
    const V3 o = horizon_origin(R, n, i, j);
    float sum = 0.0f;
    for (uint32_t k = 0u; k < R.azimuth_count; k++) {
        const float2 az = R.azimuths[k];
        const float H = horizon_walk(R.terrain, o, i, j, az.x, az.y, horizon_curvature(R, az.x, az.y), R.step_cap, levels);
        if (R.horizon) R.horizon[(size_t)k * total + n] = H;
        sum = sum + horizon_sky_term(H, az.x, az.y);
    }
    if (R.sky_view) R.sky_view[n] = 1.0f - sum / (float)R.azimuth_count;
}

}  // namespace f3d
