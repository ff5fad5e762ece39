// forge3d_amd/csrc/f3d_bvh_refit.h -- refit of a session's mesh BVH under moved vertices (f3d_session_remesh, positions only).
//
// Reference "next" piece: GpuBvhBuilder::refit (src/accel/lbvh_gpu/refit.rs, bvh_refit.wgsl) takes new triangle positions
// for an unchanged triangle count and refits the boxes bottom-up; its kernels are pending there.  Here the tree only culls
// (f3d_bvh.h: the answer is the sweep's, the triangles decide), so a refit that keeps every box CONSERVATIVE renders bit for
// bit what a tree built fresh from the moved mesh renders.  The topology -- `skip` / `leaf` words, first_child / inner,
// which triangles a leaf holds and their order -- is never written: large motion costs walk time, never the image.
//
// Three passes over a session's PRIVATE copy of vertices, leaf-order triangles and nodes (the cached mesh other sessions
// share is never written), the per-thread bodies below (host-and-device, so tests/remesh_host runs them on the CPU):
//   gather   triangle k of the leaf order (original index in v0.w) is read again from the new vertices through the indices;
//            its bounds go into the scene bounds (the kernel reduces them per wave and block, then ordered-int atomics as k_prims has them)
//   link     (first refit only) parent of every node: binary form -- children of inner node i are i + 1 and skip[i + 1];
//            four-wide form -- record first_child + k hangs in slot k of its parent, link = parent * 4 + slot
//   refit    the padding from the new bounds, by the build's own rule; leaf boxes = bounds of the leaf's triangles +- pad;
//            inner boxes = union of the children, bottom-up: the LAST thread to arrive at a node's counter does its box and
//            climbs on (one counter per node, left at zero again for the next refit).  In the four-wide form the children's
//            boxes live in the parent's slots: a record is complete when its own leaf slots and every inner child have
//            arrived, and its union goes into its slot of the parent.  Empty slots keep both planes at +inf.
// The threaded preorder BvhNode of the host SAH build (builder 3, or trees too deep for the wide walk) and the LBVH's output
// (builder 2) are one form.
#pragma once

#include "f3d_scene.h"

namespace f3d {

constexpr uint32_t kRefitNone = 0xFFFFFFFFu;
// the build's padding rule (f3d_bvh.h build_mesh_bvh, f3d_lbvh.hip): kBvhPadRel * diagonal + 4e-6 * magnitude + 1e-30
constexpr float kRefitPadRel = 1e-5f, kRefitPadMag = 4e-6f, kRefitPadMin = 1e-30f;

struct RefitParams {
    const float4 *vertices;   // the NEW positions, xyz + pad
    const uint32_t *indices;  // the session's topology (shared with the cache entry)
    float4 *tris;             // leaf order, 3 per triangle, original index in v0.w
    uint32_t tri_count;
    BvhNode *nodes;           // threaded binary form, or null
    uint32_t node_count;
    Bvh4Node *wide;           // four-wide form, or null
    uint32_t wide_count;
    uint32_t *parent;         // per node / record (link pass)
    uint32_t *counter;        // per node / record, zero between refits
    int *bounds;              // ordered-int scene bounds of THIS refit: lo[3], hi[3]
    int *bounds_next;         // the next refit's, reset by the gather pass
};

F3D_HD int refit_ordered(float f) {  // monotone float -> int (f3d_lbvh.hip ordered)
    const int i = (int)f_bits(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
F3D_HD float refit_unordered(int i) { return f_from_bits((uint32_t)(i >= 0 ? i : i ^ 0x7FFFFFFF)); }
F3D_HD void refit_bounds_reset(int *bounds) {
    for (int a = 0; a < 3; a++) {
        bounds[a] = 0x7F800000;           // ordered(+inf)
        bounds[3 + a] = (int)0x807FFFFF;  // ordered(-inf)
    }
}

// (a) triangle k of the leaf order from the new vertices; lo / hi: its bounds
F3D_HD void refit_gather_tri(const RefitParams &P, uint32_t k, float lo[3], float hi[3]) {
    const uint32_t tri = f_bits(P.tris[3u * k].w);
    const float4 a = P.vertices[P.indices[3u * tri]], b = P.vertices[P.indices[3u * tri + 1u]], c = P.vertices[P.indices[3u * tri + 2u]];
    P.tris[3u * k] = float4{a.x, a.y, a.z, f_from_bits(tri)};
    P.tris[3u * k + 1u] = float4{b.x, b.y, b.z, 0.0f};
    P.tris[3u * k + 2u] = float4{c.x, c.y, c.z, 0.0f};
    lo[0] = f_min(f_min(a.x, b.x), c.x);
    lo[1] = f_min(f_min(a.y, b.y), c.y);
    lo[2] = f_min(f_min(a.z, b.z), c.z);
    hi[0] = f_max(f_max(a.x, b.x), c.x);
    hi[1] = f_max(f_max(a.y, b.y), c.y);
    hi[2] = f_max(f_max(a.z, b.z), c.z);
}

// (b) the padding of the build for these scene bounds
F3D_HD float refit_pad(const int *bounds) {
    float diag2 = 0.0f, mag = 0.0f;
    for (int a = 0; a < 3; a++) {
        const float lo = refit_unordered(bounds[a]), hi = refit_unordered(bounds[3 + a]);
        const float d = hi - lo;
        diag2 = diag2 + d * d;
        mag = f_max(mag, f_max(f_abs(lo), f_abs(hi)));
    }
    return kRefitPadRel * f_sqrt(diag2) + kRefitPadMag * mag + kRefitPadMin;
}

// bounds of the triangles of a leaf word, +- pad
F3D_HD void refit_leaf_box(const float4 *tris, uint32_t leaf, float pad, float lo[3], float hi[3]) {
    const uint32_t first = leaf >> 3, count = leaf & 7u;
    for (int a = 0; a < 3; a++) {
        lo[a] = INFINITY;
        hi[a] = -INFINITY;
    }
    for (uint32_t v = 3u * first; v < 3u * (first + count); v++) {
        const float4 p = tris[v];
        lo[0] = f_min(lo[0], p.x);
        lo[1] = f_min(lo[1], p.y);
        lo[2] = f_min(lo[2], p.z);
        hi[0] = f_max(hi[0], p.x);
        hi[1] = f_max(hi[1], p.y);
        hi[2] = f_max(hi[2], p.z);
    }
    for (int a = 0; a < 3; a++) {
        lo[a] = lo[a] - pad;
        hi[a] = hi[a] + pad;
    }
}

// parent links, binary form: thread i
F3D_HD void refit_link_binary(const RefitParams &P, uint32_t i) {
    if (i == 0u) P.parent[0] = kRefitNone;
    if (P.nodes[i].leaf != 0u) return;
    P.parent[i + 1u] = i;
    P.parent[P.nodes[i + 1u].skip] = i;
}
// parent links, four-wide form: thread w
F3D_HD void refit_link_wide(const RefitParams &P, uint32_t w) {
    if (w == 0u) P.parent[0] = kRefitNone;
    const uint32_t first_child = P.wide[w].first_child, inner = P.wide[w].inner;
    for (uint32_t k = 0; k < inner; k++) P.parent[first_child + k] = 4u * w + k;
}

// How the bottom-up pass meets other threads.  On the device: agent-scope atomics and fences (f3d_bvh_refit.hip); on the
// host the bodies run one after the other in any order.
struct RefitSerial {
    static F3D_HD uint32_t arrive(uint32_t *counter) { return (*counter)++; }
    static F3D_HD float load(const float *p) { return *p; }
    static F3D_HD void fence() {}
};

// (c) binary form: thread i.  A leaf computes its box and climbs; the second child to arrive at a node does that node.
template <class Sync>
F3D_HD void refit_binary_node(const RefitParams &P, uint32_t i) {
    const uint32_t leaf = P.nodes[i].leaf;
    if (leaf == 0u) return;
    float lo[3], hi[3];
    refit_leaf_box(P.tris, leaf, refit_pad(P.bounds), lo, hi);
    for (int a = 0; a < 3; a++) {
        P.nodes[i].bmin[a] = lo[a];
        P.nodes[i].bmax[a] = hi[a];
    }
    for (uint32_t p = P.parent[i]; p != kRefitNone; p = P.parent[p]) {
        Sync::fence();  // this subtree's boxes before the arrival
        if (Sync::arrive(&P.counter[p]) == 0u) return;
        P.counter[p] = 0u;  // (both children are here: nobody reads it again before the next refit)
        Sync::fence();
        const BvhNode &l = P.nodes[p + 1u];
        const BvhNode &r = P.nodes[l.skip];
        for (int a = 0; a < 3; a++) {
            const float lmin = Sync::load(&l.bmin[a]), rmin = Sync::load(&r.bmin[a]);
            const float lmax = Sync::load(&l.bmax[a]), rmax = Sync::load(&r.bmax[a]);
            P.nodes[p].bmin[a] = f_min(lmin, rmin);
            P.nodes[p].bmax[a] = f_max(lmax, rmax);
        }
    }
}

// (c) four-wide form: thread w fills the leaf slots of record w; whoever completes a record -- its own thread and one
// arrival per inner child, in any order -- puts the union of its slots into its slot of the parent and arrives there.
template <class Sync>
F3D_HD void refit_wide_node(const RefitParams &P, uint32_t w) {
    {
        Bvh4Node &rec = P.wide[w];
        float pad = 0.0f;
        bool have_pad = false;
        for (uint32_t k = rec.inner; k < 4u; k++) {
            if (rec.leaf[k] == 0u) continue;  // an empty slot: both planes stay at +inf
            if (!have_pad) pad = refit_pad(P.bounds), have_pad = true;
            float lo[3], hi[3];
            refit_leaf_box(P.tris, rec.leaf[k], pad, lo, hi);
            rec.lo_x[k] = lo[0], rec.hi_x[k] = hi[0];
            rec.lo_y[k] = lo[1], rec.hi_y[k] = hi[1];
            rec.lo_z[k] = lo[2], rec.hi_z[k] = hi[2];
        }
    }
    for (uint32_t cur = w;;) {
        Bvh4Node &rec = P.wide[cur];
        const uint32_t inner = rec.inner;
        Sync::fence();
        if (Sync::arrive(&P.counter[cur]) != inner) return;  // inner + 1 arrivals complete a record
        P.counter[cur] = 0u;
        const uint32_t link = P.parent[cur];
        if (link == kRefitNone) return;
        Sync::fence();
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t k = 0; k < 4u; k++) {
            if (k >= inner && rec.leaf[k] == 0u) continue;
            lo[0] = f_min(lo[0], Sync::load(&rec.lo_x[k])), hi[0] = f_max(hi[0], Sync::load(&rec.hi_x[k]));
            lo[1] = f_min(lo[1], Sync::load(&rec.lo_y[k])), hi[1] = f_max(hi[1], Sync::load(&rec.hi_y[k]));
            lo[2] = f_min(lo[2], Sync::load(&rec.lo_z[k])), hi[2] = f_max(hi[2], Sync::load(&rec.hi_z[k]));
        }
        Bvh4Node &up = P.wide[link >> 2];
        const uint32_t slot = link & 3u;
        up.lo_x[slot] = lo[0], up.hi_x[slot] = hi[0];
        up.lo_y[slot] = lo[1], up.hi_y[slot] = hi[1];
        up.lo_z[slot] = lo[2], up.hi_z[slot] = hi[2];
        cur = link >> 2;
    }
}

#if defined(__HIPCC__)
// f3d_bvh_refit.hip: the passes on `stream`.  link: also derive the parent links (the first refit of a private copy).
hipError_t launch_bvh_refit(const RefitParams &P, bool link, hipStream_t stream);
#endif

}  // namespace f3d
