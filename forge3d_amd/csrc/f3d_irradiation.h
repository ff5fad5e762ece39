// forge3d_amd/csrc/f3d_irradiation.h -- irradiation rasters on a live session (f3d_session_irradiation): what one lane of
// k_irradiation does.  Per DEM sample, the energy the direct beam delivers over a sun track: every sun position weighted by
// its irradiance and by the cosine of incidence on the local slope, counted only where the visibility rasters' ray toward it
// is unblocked (the r.sun / "solar radiation" raster of a GIS).  A facet that faces away from a sun position needs no ray:
// that term is settled before any march.
//
// THE CONTRACT.  All arithmetic is f32, one rounding per written operation, and NO fma in anything below (plane_at is the
// march's own and the one exception), so that NumPy reproduces it from the DEM bit for bit (f3d_horizon.h horizon_sky_term
// is done the same way).
//
// Sample and origin: exactly the visibility rasters' (f3d_raster.h raster_origin).  Sample n = r * cols + c of the region is
// DEM sample (j = row0 + r, i = col0 + c), and its rays start on the lifted lattice point
//     o = (plane_at(origin_x, i, spacing_x), hgt(i, j) + lift, plane_at(origin_z, j, spacing_z))
// where hgt is the sample as the session holds it: the corner of the leaf table's record, exaggeration applied.
//
// Surface gradient of sample (i, j), once per lane: central differences, one-sided on the border.  With w = cell_w + 1,
// h = cell_h + 1 (a DEM is at least 2 x 2, so iE > iW and jS > jN):
//     iW = i > 0 ? i - 1 : i,   iE = i + 1 < w ? i + 1 : i,   jN = j > 0 ? j - 1 : j,   jS = j + 1 < h ? j + 1 : j
//     run_x = plane_at(origin_x, iE, spacing_x) - plane_at(origin_x, iW, spacing_x),   run_z likewise
//     gx = (hgt(iE, j) - hgt(iW, j)) / run_x,   gz = (hgt(i, jS) - hgt(i, jN)) / run_z,   q = (gx gx + gz gz) + 1
// With HORIZONTAL gx = gz = 0 and q = 1 (the beam on a horizontal plane) and the four loads are skipped.  The unit normal is
// (-gx, 1, -gz) / sqrt(q), each component its own division.
//
// Direction k is (x, y, z, wt): a direction TOWARD the sun as given (it need not be unit) and a weight (W/m^2 x hours, say):
//     l2 = (x x + y y) + z z,   m = (y - gx x) - gz z,   c = m / sqrt(q l2)          (the cosine of incidence)
//     go = query_ray_good(o, 0, d, 1e30) && wt > 0 && c > 0                          (a NaN anywhere: false)
// and if the ray (o, tmin 0, d = (x, y, z), tmax 1e30) is unblocked -- occluded() under the raster's curvature policy --
//     sum = sum + wt * c,   seen += 1.
// A facet turned away from the sun, a zero-weight term and a refused direction contribute 0 AND NEVER MARCH.
//
// irradiation_term() is ONE direction of ONE lane, shaped as raster_visible is: everything that decides `go` comes first and
// has no wave primitive in it, then a single `if (go)` holds the march -- two call sites chosen by a wave-uniform flag.  The
// lanes that do not go are outside that region for this direction; every lane that goes is in the same march of the same
// direction.  The loop over the directions is the caller's: k_irradiation's has a wave-uniform trip count.
#pragma once

#include "f3d_query.h"
#include "f3d_walk.h"

namespace f3d {

// the gradient of a lane's sample: (gx, gz) and q = gx^2 + gz^2 + 1
struct IrradiationSlope {
    float gx, gz, q;
};

// DEM sample (i, j) of sample n of the region, and its lifted lattice point
F3D_HD V3 irradiation_origin(const IrradiationParams &R, uint32_t n, uint32_t &i, uint32_t &j) {
    return lattice_point(R.frame.terrain, R.row0, R.col0, R.cols, n, R.lift, i, j);
}

F3D_HD IrradiationSlope irradiation_slope(const IrradiationParams &R, uint32_t i, uint32_t j) {
    if (R.horizontal != 0u) return IrradiationSlope{0.0f, 0.0f, 1.0f};
    const TerrainDev &T = R.frame.terrain;
    const uint32_t w = T.cell_w + 1u, h = T.cell_h + 1u;
    const uint32_t iW = i > 0u ? i - 1u : i, iE = i + 1u < w ? i + 1u : i, jN = j > 0u ? j - 1u : j, jS = j + 1u < h ? j + 1u : j;
    const float run_x = plane_at(T.origin_x, iE, T.spacing_x) - plane_at(T.origin_x, iW, T.spacing_x);
    const float run_z = plane_at(T.origin_z, jS, T.spacing_z) - plane_at(T.origin_z, jN, T.spacing_z);
    const float gx = (lattice_height(T, iE, j) - lattice_height(T, iW, j)) / run_x;
    const float gz = (lattice_height(T, i, jS) - lattice_height(T, i, jN)) / run_z;
    return IrradiationSlope{gx, gz, (gx * gx + gz * gz) + 1.0f};
}

F3D_HD V3 irradiation_normal(IrradiationSlope s) {
    const float len = f_sqrt(s.q);
    return V3{-s.gx / len, 1.0f / len, -s.gz / len};
}

// One lane, one direction: what the sample's sum takes from it; `lit`: the term contributed.  Every lane of the wave that has
// a sample calls it for the same direction together (see the header).
template <class Pending>
F3D_HD float irradiation_term(const IrradiationParams &R, V3 o, IrradiationSlope s, float4 dir, Pending &pend, bool &lit) {
    const FrameParams &P = R.frame;
    const V3 d{dir.x, dir.y, dir.z};
    const float l2 = (dir.x * dir.x + dir.y * dir.y) + dir.z * dir.z;
    const float m = (dir.y - s.gx * dir.x) - s.gz * dir.z;
    const float c = m / f_sqrt(s.q * l2);
    const bool go = query_ray_good(o, 0.0f, d, 1e30f) && dir.w > 0.0f && c > 0.0f;
    bool blocked = true;
    if (go) blocked = R.curved != 0u ? occluded(P, o, 0.0f, d, 1e30f, true, pend) : occluded(P, o, 0.0f, d, 1e30f, false, pend);
    lit = !blocked;
    return lit ? dir.w * c : 0.0f;
}

}  // namespace f3d
