// forge3d_amd/csrc/f3d_raster.h -- DEM visibility rasters on a live session (f3d_session_raster): what one lane of k_raster
// does.  The reference's terrain.viewshed and terrain.shadow_mask ask one question of every DEM sample; here the device
// builds the rays from the terrain it already holds and marches them with the frame kernels' occluded(), so no ray list
// crosses the bus: one lane owns a sample of the region, keeps its origin in registers and loops over the targets.
//
// All arithmetic is f32, one rounding per written operation.  Sample n = r * cols + c of the region is DEM sample
// (j = row0 + r, i = col0 + c); its ray starts on the lifted lattice point
//     o = (plane_at(origin_x, i, spacing_x), h(i, j) + lift, plane_at(origin_z, j, spacing_z))
// where h is the sample as the session holds it -- a corner of the leaf table's record, exaggeration applied -- and plane_at
// is the march's own fma, so the point lies on the lattice the march steps over.  Target (x, y, z, w):
//   TOWARD_POINT     dx = x - o.x, dz = z - o.z, hd2 = dx dx + dz dz, dy = y - o.y, and under the curvature policy (CURVED on
//                    a scene whose curvature is enabled) dy = dy - hd2 * inv_two_r_prime: the curved march adds
//                    t^2 hd2 inv_two_r_prime to the ray's height (f3d_trace.h height_at), so the point's own height above its
//                    datum is reached at t = 1.  Ray (o, tmin 0, d = (dx, dy, dz), tmax 1).  w > 0 is a maximum horizontal
//                    distance: hd2 > w w answers "not visible" with no march.
//   ALONG_DIRECTION  d = (x, y, z) as given, tmin 0, tmax 1e30.
// A ray query_ray_good (f3d_query.h) refuses -- a non-finite component, a zero direction: the observer standing exactly on
// the lifted sample -- answers 0 like a blocked one, before any march.
//
// The marches vote (flush, share: f3d_march.h), and a sample's lane may be cut off or refused for one target and march for
// the next.  raster_visible() is therefore ONE target of ONE lane, shaped as query_lane is: everything that decides whether
// the lane marches comes first and has no wave primitive in it, then a single `if (go)` holds the march -- two call sites,
// chosen by a wave-uniform flag.  The lanes that do not go are outside that region for this target (on the device their EXEC
// bit is off and the ballots do not see them; on the host they have left the wave) and every lane that goes is in the same
// march of the same target.  The loop over the targets is the caller's: k_raster's has a wave-uniform trip count and meets
// again after each target, where the wave's ballot becomes the mask word; tests/raster_host runs a wave per target.
#pragma once

#include "f3d_query.h"
#include "f3d_walk.h"

namespace f3d {

// the lifted lattice point of sample n of the region
F3D_HD V3 raster_origin(const RasterParams &R, uint32_t n) {
    uint32_t i, j;
    return lattice_point(R.frame.terrain, R.row0, R.col0, R.cols, n, R.lift, i, j);
}

// One lane, one target: is the target visible (the direction unblocked) from o?  Every lane of the wave that has a sample
// calls it for the same target together (see the header).
template <class Pending>
F3D_HD bool raster_visible(const RasterParams &R, V3 o, float4 target, Pending &pend) {
    const FrameParams &P = R.frame;
    V3 d{target.x, target.y, target.z};
    float tmax = 1e30f;
    bool go = true;
    if (R.mode == kRasterTowardPoint) {
        const float dx = target.x - o.x, dz = target.z - o.z;
        const float hd2 = dx * dx + dz * dz;
        float dy = target.y - o.y;
        if (R.curved != 0u && P.terrain.curvature_enabled != 0u) dy = dy - hd2 * P.terrain.inv_two_r_prime;
        d = V3{dx, dy, dz};
        tmax = 1.0f;
        go = !(target.w > 0.0f && hd2 > target.w * target.w);
    }
    go = go && query_ray_good(o, 0.0f, d, tmax);
    bool blocked = true;
    if (go) blocked = R.curved != 0u ? occluded(P, o, 0.0f, d, tmax, true, pend) : occluded(P, o, 0.0f, d, tmax, false, pend);
    return !blocked;
}

}  // namespace f3d
