// forge3d_amd/csrc/f3d_query.h -- ray queries on a live session (f3d_session_query): what one lane of k_query does.
//
// A session holds the only current copy of its scene (the terrain after a re-terrain, the mesh after a re-mesh, the camera
// after a re-aim); a query asks that scene a question with the frame kernels' own device functions and changes nothing a
// frame launch reads:
//   mode 0  closest hit   closest_hit(P, o, tmin, d, tmax, pend): the reference's intersect_hybrid, curvature off, mesh and
//                         terrain; the ray is used as given (t is in units of |d|, nothing is normalised)
//   mode 1  occlusion     occluded(P, o, tmin, d, tmax, curved, pend): the any-hit march of the shadow and IBL rays
//   mode 2  pixels        the centre ray of pixel (gx, gy) of the session's CURRENT camera, traced as the G-buffer pass traces
//                         it (origin cam.origin, tmin 1e-3, tmax 1e30): the bits that pass stores in the depth and normal AOVs.
//                         The march starts at the root, as the G-buffer pass's does.
// TERRAIN_ONLY is the host's: it hands the kernel uniforms whose mesh.traversal_mode says "terrain only" and launches the
// instantiation without the mesh walk.
//
// A BAD ray -- a non-finite component, a direction whose squared length is not a positive finite f32 (zero, or so small or
// large that it leaves the f32 range), tmax <= tmin; in mode 2 a pixel outside the image -- is answered as a miss by its lane
// BEFORE any walk or march starts: the march's loops are bounded by the ray's own interval arithmetic, and a NaN in it
// compares false everywhere.  No input keeps a wave running.  The host form and the device form run this same code.
//
// The body is host-and-device: tests/query_host runs it on the CPU over whole 64-lane waves against the oracle.
#pragma once

#include "f3d_shade.h"

namespace f3d {

constexpr uint32_t kQueryNoPrimitive = 0xFFFFFFFFu;

F3D_HD bool query_finite(float v) { return (f_bits(v) & 0x7F800000u) != 0x7F800000u; }

// may this ray be walked?  (see the header: everything else is a miss before any march)
F3D_HD bool query_ray_good(V3 o, float tmin, V3 d, float tmax) {
    const bool finite = query_finite(o.x) && query_finite(o.y) && query_finite(o.z) && query_finite(d.x) && query_finite(d.y) &&
                        query_finite(d.z) && query_finite(tmin) && query_finite(tmax);
    const float len2 = d.x * d.x + d.y * d.y + d.z * d.z;
    return finite && len2 > 0.0f && query_finite(len2) && tmax > tmin;
}

// One lane, one ray: entry i of the batch.  Every lane of the wave that has a ray calls it (the marches vote).
template <class Pending>
F3D_HD void query_lane(const QueryParams &Q, uint32_t i, Pending &pend) {
    const FrameParams &P = Q.frame;
    V3 o, d;
    float tmin, tmax;
    bool good;
    if (Q.mode == kQueryPixels) {
        const uint2 px = Q.pixels[i];
        good = px.x < P.cam.width && px.y < P.cam.height;
        o = P.cam.origin;
        d = good ? camera_dir(P.cam, px.x, px.y, 0.0f, 0.0f) : V3{0.0f, 0.0f, 0.0f};
        tmin = 1e-3f;
        tmax = 1e30f;
    } else {
        const float4 a = Q.rays[2u * (size_t)i], b = Q.rays[2u * (size_t)i + 1u];
        o = V3{a.x, a.y, a.z};
        d = V3{b.x, b.y, b.z};
        tmin = a.w;
        tmax = b.w;
        good = query_ray_good(o, tmin, d, tmax);
    }
    SurfaceHit hit;
    hit.kind = 0u;
    hit.t = f_from_bits(0x7fc00000u);
    hit.p = V3{0.0f, 0.0f, 0.0f};
    hit.n = V3{0.0f, 0.0f, 0.0f};
    uint32_t primitive = kQueryNoPrimitive;
    if (good) {
        if (Q.mode == kQueryOccluded) {
            // (the curvature policy is a compile-time constant of the march: two call sites, the flag is wave-uniform)
            const bool blocked = Q.curved != 0u ? occluded(P, o, tmin, d, tmax, true, pend) : occluded(P, o, tmin, d, tmax, false, pend);
            hit.kind = blocked ? 1u : 0u;
        } else {
            uint32_t what = kQueryNoPrimitive;
            const SurfaceHit h = closest_hit(P, o, tmin, d, tmax, pend, 0.0f, 0u, &what);
            if (h.kind != 0u) {
                hit = h;
                primitive = what;
            }
        }
    }
    if (Q.kind) Q.kind[i] = hit.kind;
    if (Q.t) Q.t[i] = hit.t;
    if (Q.normal) {
        Q.normal[3u * (size_t)i] = hit.n.x;
        Q.normal[3u * (size_t)i + 1u] = hit.n.y;
        Q.normal[3u * (size_t)i + 2u] = hit.n.z;
    }
    if (Q.position) {
        Q.position[3u * (size_t)i] = hit.p.x;
        Q.position[3u * (size_t)i + 1u] = hit.p.y;
        Q.position[3u * (size_t)i + 2u] = hit.p.z;
    }
    if (Q.primitive) Q.primitive[i] = primitive;
    if (Q.direction) {
        Q.direction[3u * (size_t)i] = d.x;
        Q.direction[3u * (size_t)i + 1u] = d.y;
        Q.direction[3u * (size_t)i + 2u] = d.z;
    }
}

}  // namespace f3d
