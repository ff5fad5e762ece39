// tests/remesh_host/remesh_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_remesh_host.py compiles it).
// The refit passes of a re-mesh (f3d_bvh_refit.h: what k_remesh_gather / k_remesh_link / k_remesh_refit_* run per thread)
// on the host, over trees built by the product's own builders from a mesh at positions A, refitted to positions B:
//   form 1  the threaded binary tree of build_mesh_bvh
//   form 2  the same tree four children wide (collapse_bvh4; a tree too deep for it stays binary and says so)
//   form 3  a binary tree in the GPU LBVH's output form: Morton-sorted triangles, leaves of <= 4 in sorted order, a node
//           array longer than the tree (f3d_lbvh.hip allocates 2n - 1 records)
// The bodies run one "thread" after the other in a shuffled order (RefitSerial), optionally after an earlier refit to
// other positions, so that what a refit leaves behind -- counters, the other set of bounds -- is part of the test.
// Checked: (i) the boxes -- leaves hold their triangles by the build's padding for the NEW bounds, parents hold their
// children, empty wide slots keep both planes at +inf, no topology word changed, the leaf-order triangles are the moved
// ones; (ii) the walks -- closest hit (hit, t, normal bit for bit) and any hit on the refitted tree against the sweep over
// the moved mesh and against a tree built fresh from it.  (An any-hit walk answers "is there a triangle": it stops at the
// first one it accepts, in visiting order, so its t and normal are not the sweep's and only the answer is compared.)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../forge3d_amd/csrc/f3d_setup.h"
#include "../../forge3d_amd/csrc/f3d_meshgrid.h"
#include "../../forge3d_amd/csrc/f3d_shade.h"
#include "../../forge3d_amd/csrc/f3d_bvh.h"
#include "../../forge3d_amd/csrc/f3d_bvh_refit.h"

using namespace f3d;

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {  // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double uniform(double a, double b) { return a + (b - a) * uniform(); }
};

struct Stack {
    uint32_t words[kBvh4MaxLevels + 1u];
    void stack_put(uint32_t level, uint32_t word) { words[level] = word; }
    uint32_t stack_get(uint32_t level) const { return words[level]; }
};

struct Tree {
    std::vector<BvhNode> nodes;  // may be longer than node_count (form 3)
    uint32_t node_count = 0;
    std::vector<Bvh4Node> wide;
    std::vector<float> tris;
};

uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

float build_pad(const float *verts, const uint32_t *idx, uint32_t index_count) {  // the rule of build_mesh_bvh
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < index_count; i++)
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min(lo[a], verts[3u * (size_t)idx[i] + a]);
            hi[a] = std::max(hi[a], verts[3u * (size_t)idx[i] + a]);
        }
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    float mag = 0.0f;
    for (int a = 0; a < 3; a++) mag = std::max(mag, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
    return kBvhPadRel * std::sqrt(dx * dx + dy * dy + dz * dz) + 4e-6f * mag + 1e-30f;
}

// form 3: the output form of the GPU LBVH over Morton-sorted triangles (median splits stand in for the Karras splits)
void emit_sorted(Tree &t, const std::vector<uint32_t> &order, const float *verts, const uint32_t *idx, uint32_t first, uint32_t count, float pad) {
    const uint32_t me = (uint32_t)t.node_count++;
    BvhNode n{};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t k = first; k < first + count; k++)
        for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], verts[3u * (size_t)idx[3u * order[k] + v] + a]);
                hi[a] = std::max(hi[a], verts[3u * (size_t)idx[3u * order[k] + v] + a]);
            }
    for (int a = 0; a < 3; a++) {
        n.bmin[a] = lo[a] - pad;
        n.bmax[a] = hi[a] + pad;
    }
    if (count <= 4u) {
        n.leaf = (first << 3) | count;
    } else {
        const uint32_t left = count / 2u + (count % 3u == 0u ? 1u : 0u);  // (not always the middle)
        emit_sorted(t, order, verts, idx, first, left, pad);
        emit_sorted(t, order, verts, idx, first + left, count - left, pad);
    }
    n.skip = t.node_count;
    t.nodes[me] = n;
}

Tree build_tree(const float *verts, uint32_t vertex_count, const uint32_t *idx, uint32_t index_count, int form, int *form_used) {
    Tree t;
    const uint32_t ntri = index_count / 3u;
    *form_used = form;
    if (form == 3) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        std::vector<float> c(3u * (size_t)ntri);
        for (uint32_t k = 0; k < ntri; k++)
            for (int a = 0; a < 3; a++) {
                float l = INFINITY, h = -INFINITY;
                for (int v = 0; v < 3; v++) {
                    l = std::min(l, verts[3u * (size_t)idx[3u * k + v] + a]);
                    h = std::max(h, verts[3u * (size_t)idx[3u * k + v] + a]);
                }
                c[3u * k + a] = 0.5f * (l + h);
                lo[a] = std::min(lo[a], c[3u * k + a]);
                hi[a] = std::max(hi[a], c[3u * k + a]);
            }
        std::vector<uint64_t> keys(ntri);
        for (uint32_t k = 0; k < ntri; k++) {
            uint32_t g[3];
            for (int a = 0; a < 3; a++) {
                const float u = std::min(std::max((c[3u * k + a] - lo[a]) / std::max(hi[a] - lo[a], 1e-6f), 0.0f), 1.0f);
                g[a] = std::min((uint32_t)(u * 1023.0f), 1023u);
            }
            keys[k] = ((uint64_t)(expand_bits(g[0]) | (expand_bits(g[1]) << 1) | (expand_bits(g[2]) << 2)) << 32) | k;
        }
        std::sort(keys.begin(), keys.end());
        std::vector<uint32_t> order(ntri);
        for (uint32_t k = 0; k < ntri; k++) order[k] = (uint32_t)(keys[k] & 0xFFFFFFFFull);
        BvhNode junk;
        std::memset(&junk, 0xA5, sizeof junk);
        t.nodes.assign(2u * (size_t)ntri - 1u, junk);  // (the records past the tree are never read)
        emit_sorted(t, order, verts, idx, 0u, ntri, build_pad(verts, idx, index_count));
        t.tris.resize(12u * (size_t)ntri);
        for (uint32_t k = 0; k < ntri; k++)
            for (int v = 0; v < 3; v++) {
                const float *p = verts + 3u * (size_t)idx[3u * order[k] + v];
                float w = 0.0f;
                if (v == 0) std::memcpy(&w, &order[k], 4);
                const float rec[4] = {p[0], p[1], p[2], w};
                std::memcpy(&t.tris[12u * (size_t)k + 4u * v], rec, sizeof rec);
            }
        return t;
    }
    MeshBvh b = build_mesh_bvh(verts, vertex_count, idx, index_count);
    if (form == 2) {
        t.wide = collapse_bvh4(b);
        if (t.wide.empty()) *form_used = 1;
    }
    t.nodes = std::move(b.nodes);
    t.node_count = (uint32_t)t.nodes.size();
    t.tris = std::move(b.tris);
    return t;
}

MeshDev mesh_dev(const std::vector<float> &v4, uint32_t vertex_count, const uint32_t *idx, uint32_t index_count, const Tree *t) {
    MeshDev M{};
    M.vertices = (const float4 *)v4.data();
    M.indices = idx;
    M.vertex_count = vertex_count;
    M.index_count = index_count;
    M.traversal_mode = 0u;
    if (t) {
        M.bvh_tris = (const float4 *)t->tris.data();
        if (!t->wide.empty()) {
            M.bvh4_nodes = t->wide.data();
            M.bvh4_node_count = (uint32_t)t->wide.size();
        } else {
            M.bvh_nodes = t->nodes.data();
            M.bvh_node_count = t->node_count;
        }
    }
    return M;
}

// one refit of `t` to the positions v4 (xyz + pad), the bodies in a shuffled order; state: parent, counter, bounds[12], refits
struct RefitState {
    std::vector<uint32_t> parent, counter;
    int bounds[12];
    uint32_t refits = 0;
};

void refit(Tree &t, RefitState &st, const std::vector<float> &v4, const uint32_t *idx, uint32_t index_count, Rng &rng) {
    const bool wide = !t.wide.empty();
    const uint32_t n = wide ? (uint32_t)t.wide.size() : t.node_count;
    const bool first = st.refits == 0u;
    if (first) {
        st.parent.assign(n, 0xDEADBEEFu);
        st.counter.assign(n, 0u);
        refit_bounds_reset(st.bounds);
        refit_bounds_reset(st.bounds + 6);
    }
    RefitParams P{};
    P.vertices = (const float4 *)v4.data();
    P.indices = idx;
    P.tris = (float4 *)t.tris.data();
    P.tri_count = index_count / 3u;
    if (wide) {
        P.wide = t.wide.data();
        P.wide_count = n;
    } else {
        P.nodes = t.nodes.data();
        P.node_count = n;
    }
    P.parent = st.parent.data();
    P.counter = st.counter.data();
    P.bounds = st.bounds + 6u * (st.refits & 1u);
    P.bounds_next = st.bounds + 6u * ((st.refits & 1u) ^ 1u);
    auto shuffled = [&](uint32_t count) {
        std::vector<uint32_t> order(count);
        std::iota(order.begin(), order.end(), 0u);
        for (uint32_t i = count; i > 1u; i--) std::swap(order[i - 1u], order[rng.next() % i]);
        return order;
    };
    refit_bounds_reset(P.bounds_next);  // (thread 0 of the gather kernel)
    for (uint32_t k : shuffled(P.tri_count)) {
        float lo[3], hi[3];
        refit_gather_tri(P, k, lo, hi);
        for (int a = 0; a < 3; a++) {  // (the kernel: wave reduction, then atomicMin / atomicMax on the ordered ints)
            P.bounds[a] = std::min(P.bounds[a], refit_ordered(lo[a]));
            P.bounds[3 + a] = std::max(P.bounds[3 + a], refit_ordered(hi[a]));
        }
    }
    if (first)
        for (uint32_t i : shuffled(n)) wide ? refit_link_wide(P, i) : refit_link_binary(P, i);
    for (uint32_t i : shuffled(n)) wide ? refit_wide_node<RefitSerial>(P, i) : refit_binary_node<RefitSerial>(P, i);
    st.refits++;
}

bool holds(const float lo[3], const float hi[3], const float in_lo[3], const float in_hi[3]) {
    for (int a = 0; a < 3; a++)
        if (!(lo[a] <= in_lo[a] && hi[a] >= in_hi[a])) return false;
    return true;
}
void slot_box(const Bvh4Node &r, uint32_t k, float lo[3], float hi[3]) {
    lo[0] = r.lo_x[k], lo[1] = r.lo_y[k], lo[2] = r.lo_z[k];
    hi[0] = r.hi_x[k], hi[1] = r.hi_y[k], hi[2] = r.hi_z[k];
}
// does the box hold the triangles of a leaf word by at least pad?
bool holds_leaf(const float lo[3], const float hi[3], const std::vector<float> &tris, uint32_t leaf, float pad) {
    const uint32_t first = leaf >> 3, count = leaf & 7u;
    for (uint32_t v = 3u * first; v < 3u * (first + count); v++)
        for (int a = 0; a < 3; a++) {
            const float p = tris[4u * (size_t)v + a];
            if (!(lo[a] <= p - pad && hi[a] >= p + pad)) return false;
        }
    return true;
}

}  // namespace

// out: [0] leaf boxes that do not hold their triangles by the pad, [1] parents that do not hold a child, [2] empty wide slots
// not (+inf, +inf), [3] topology words changed, [4] leaf-order triangles that are not the moved ones, [5] counters not back at
// zero, [6] pad bits differ from the build's rule, [7] closest-hit rays that differ from the sweep, [8] any-hit answers that
// differ from the sweep's, [9] closest-hit rays that differ from the fresh tree's, [10] any-hit answers that differ from the
// fresh tree's, [11] aimed rays, [12] aimed rays that hit, [13] rays, [14] rays that hit, [15] form used, [16] nodes / records
extern "C" int remesh_check(const float *verts_a, const float *verts_b, uint32_t vertex_count, const uint32_t *idx, uint32_t index_count,
                            int form, int twice, uint32_t aimed, uint32_t random, uint64_t seed, uint64_t *out) {
    for (int i = 0; i < 17; i++) out[i] = 0;
    if (index_count < 3u || index_count % 3u != 0u) return 1;
    for (uint32_t i = 0; i < index_count; i++)
        if (idx[i] >= vertex_count) return 1;
    Rng rng{seed};
    int form_used = form, fresh_form = form;
    Tree t = build_tree(verts_a, vertex_count, idx, index_count, form, &form_used);
    const Tree before = t;
    const std::vector<float> b4 = pad_rgb_to_rgba(verts_b, vertex_count, 0.0f);
    RefitState st;
    if (twice) {  // an earlier refit to other positions: A mirrored, scaled and pushed aside
        std::vector<float> other(3u * (size_t)vertex_count);
        for (size_t i = 0; i < other.size(); i++) other[i] = -2.5f * verts_a[i] + (float)(i % 3u) * 17.0f;
        refit(t, st, pad_rgb_to_rgba(other.data(), vertex_count, 0.0f), idx, index_count, rng);
    }
    refit(t, st, b4, idx, index_count, rng);
    const bool wide = !t.wide.empty();
    out[15] = (uint64_t)form_used;
    out[16] = wide ? t.wide.size() : t.node_count;

    // ---- (i) the boxes ----
    const float pad = build_pad(verts_b, idx, index_count);
    const int *bounds = st.bounds + 6u * ((st.refits - 1u) & 1u);
    const float pad_refit = refit_pad(bounds);
    out[6] = std::memcmp(&pad, &pad_refit, 4) != 0;
    for (uint32_t c : st.counter) out[5] += c != 0u;
    for (uint32_t k = 0; k < index_count / 3u; k++) {
        uint32_t tri, tri0;
        std::memcpy(&tri, &t.tris[12u * (size_t)k + 3u], 4);
        std::memcpy(&tri0, &before.tris[12u * (size_t)k + 3u], 4);
        bool same = tri == tri0 && tri < index_count / 3u;
        for (int v = 0; v < 3 && same; v++) {
            const float want[4] = {verts_b[3u * (size_t)idx[3u * tri + v]], verts_b[3u * (size_t)idx[3u * tri + v] + 1u],
                                   verts_b[3u * (size_t)idx[3u * tri + v] + 2u], 0.0f};
            same = std::memcmp(&t.tris[12u * (size_t)k + 4u * v], want, v == 0 ? 12 : 16) == 0;
        }
        out[4] += !same;
    }
    if (wide) {
        for (size_t w = 0; w < t.wide.size(); w++) {
            const Bvh4Node &r = t.wide[w], &r0 = before.wide[w];
            out[3] += std::memcmp(r.leaf, r0.leaf, sizeof r.leaf) != 0 || r.first_child != r0.first_child || r.inner != r0.inner ||
                      r.pad0 != r0.pad0 || r.pad1 != r0.pad1;
            for (uint32_t k = 0; k < 4u; k++) {
                float lo[3], hi[3];
                slot_box(r, k, lo, hi);
                if (k < r.inner) {
                    const Bvh4Node &c = t.wide[r.first_child + k];
                    for (uint32_t j = 0; j < 4u; j++) {
                        if (j >= c.inner && c.leaf[j] == 0u) continue;
                        float clo[3], chi[3];
                        slot_box(c, j, clo, chi);
                        out[1] += !holds(lo, hi, clo, chi);
                    }
                } else if (r.leaf[k] != 0u) {
                    out[0] += !holds_leaf(lo, hi, t.tris, r.leaf[k], pad);
                } else {
                    for (int a = 0; a < 3; a++) out[2] += !(lo[a] == INFINITY && hi[a] == INFINITY);
                }
            }
        }
    } else {
        for (uint32_t i = 0; i < t.node_count; i++) {
            const BvhNode &n = t.nodes[i], &n0 = before.nodes[i];
            out[3] += n.skip != n0.skip || n.leaf != n0.leaf;
            if (n.leaf != 0u) {
                out[0] += !holds_leaf(n.bmin, n.bmax, t.tris, n.leaf, pad);
            } else {
                const BvhNode &l = t.nodes[i + 1u], &r = t.nodes[l.skip];
                out[1] += !holds(n.bmin, n.bmax, l.bmin, l.bmax);
                out[1] += !holds(n.bmin, n.bmax, r.bmin, r.bmax);
            }
        }
        for (size_t i = t.node_count; i < t.nodes.size(); i++) out[3] += std::memcmp(&t.nodes[i], &before.nodes[i], sizeof(BvhNode)) != 0;
    }

    // ---- (ii) the walks ----
    const Tree fresh = build_tree(verts_b, vertex_count, idx, index_count, form_used, &fresh_form);
    const MeshDev sweep = mesh_dev(b4, vertex_count, idx, index_count, nullptr);
    const MeshDev refitted = mesh_dev(b4, vertex_count, idx, index_count, &t);
    const MeshDev rebuilt = mesh_dev(b4, vertex_count, idx, index_count, &fresh);
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = refit_unordered(bounds[a]);
        hi[a] = refit_unordered(bounds[3 + a]);
    }
    const double cx = 0.5 * ((double)lo[0] + hi[0]), cy = 0.5 * ((double)lo[1] + hi[1]), cz = 0.5 * ((double)lo[2] + hi[2]);
    const double radius = 0.5 * std::sqrt(((double)hi[0] - lo[0]) * ((double)hi[0] - lo[0]) + ((double)hi[1] - lo[1]) * ((double)hi[1] - lo[1]) +
                                          ((double)hi[2] - lo[2]) * ((double)hi[2] - lo[2]));
    const uint32_t total = aimed + random;
    std::vector<float> rays(6u * (size_t)total);
    for (uint32_t r = 0; r < total; r++) {
        double d[3];
        double len2;
        do {
            for (double &x : d) x = rng.uniform(-1.0, 1.0);
            len2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        } while (len2 < 1e-4 || len2 > 1.0);
        const double inv = 1.0 / std::sqrt(len2);
        double o[3], dir[3];
        if (r < aimed) {  // from outside towards a point of the moved mesh's bounding box
            const double dist = rng.uniform(1.2, 3.0) * radius + 1.0;
            o[0] = cx + d[0] * inv * dist, o[1] = cy + d[1] * inv * dist, o[2] = cz + d[2] * inv * dist;
            const double target[3] = {rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), rng.uniform(lo[2], hi[2])};
            double l = 0.0;
            for (int a = 0; a < 3; a++) {
                dir[a] = target[a] - o[a];
                l += dir[a] * dir[a];
            }
            for (double &x : dir) x /= std::sqrt(l);
        } else {  // anywhere, any direction (origins inside the mesh's bounds included)
            const double reach = 2.0 * radius + 10.0;
            o[0] = cx + rng.uniform(-reach, reach), o[1] = cy + rng.uniform(-reach, reach), o[2] = cz + rng.uniform(-reach, reach);
            for (int a = 0; a < 3; a++) dir[a] = d[a] * inv;
        }
        for (int a = 0; a < 3; a++) {
            rays[6u * (size_t)r + a] = (float)o[a];
            rays[6u * (size_t)r + 3u + a] = (float)dir[a];
        }
    }
    uint64_t bad_closest = 0, bad_any = 0, bad_fresh = 0, bad_fresh_any = 0, hits = 0, aimed_hits = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : bad_closest, bad_any, bad_fresh, bad_fresh_any, hits, aimed_hits)
    for (long r = 0; r < (long)total; r++) {
        const V3 o{rays[6u * (size_t)r], rays[6u * (size_t)r + 1u], rays[6u * (size_t)r + 2u]};
        const V3 d{rays[6u * (size_t)r + 3u], rays[6u * (size_t)r + 4u], rays[6u * (size_t)r + 5u]};
        const float tmin = 1e-4f, tmax = 1e30f;
        Stack stk{};
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, ta = 0.0f;
        V3 n0{0, 0, 0}, n1{0, 0, 0}, n2{0, 0, 0}, na{0, 0, 0};
        const bool h0 = mesh_sweep(sweep, o, tmin, d, tmax, t0, n0);
        const bool h1 = mesh_closest(refitted, o, tmin, d, tmax, t1, n1, stk);
        const bool h2 = mesh_closest(rebuilt, o, tmin, d, tmax, t2, n2, stk);
        const bool a1 = mesh_any(refitted, o, tmin, d, tmax, ta, na, stk);
        const bool a2 = mesh_any(rebuilt, o, tmin, d, tmax, ta, na, stk);
        const auto same = [](bool ha, float tta, V3 nna, bool hb, float ttb, V3 nnb) {
            if (ha != hb) return false;
            if (!ha) return true;
            return f_bits(tta) == f_bits(ttb) && f_bits(nna.x) == f_bits(nnb.x) && f_bits(nna.y) == f_bits(nnb.y) && f_bits(nna.z) == f_bits(nnb.z);
        };
        bad_closest += !same(h0, t0, n0, h1, t1, n1);
        bad_fresh += !same(h2, t2, n2, h1, t1, n1);
        bad_any += a1 != h0;
        bad_fresh_any += a1 != a2;
        hits += h0;
        aimed_hits += h0 && r < (long)aimed;
    }
    out[7] = bad_closest;
    out[8] = bad_any;
    out[9] = bad_fresh;
    out[10] = bad_fresh_any;
    out[11] = aimed;
    out[12] = aimed_hits;
    out[13] = total;
    out[14] = hits;
    return 0;
}

// The comparison can fail: the same checks over a tree whose boxes were NOT refitted (the triangles moved, the boxes stayed).
// out as remesh_check's [7], [8] and [12]: closest-hit rays and any-hit answers that differ from the sweep, aimed hits.
extern "C" int remesh_stale(const float *verts_a, const float *verts_b, uint32_t vertex_count, const uint32_t *idx, uint32_t index_count,
                            int form, uint32_t aimed, uint64_t seed, uint64_t *out) {
    out[0] = out[1] = out[2] = 0;
    Rng rng{seed};
    int form_used = form;
    Tree t = build_tree(verts_a, vertex_count, idx, index_count, form, &form_used);
    const std::vector<float> b4 = pad_rgb_to_rgba(verts_b, vertex_count, 0.0f);
    for (uint32_t k = 0; k < index_count / 3u; k++) {  // the triangles move (the gather pass alone)
        uint32_t tri;
        std::memcpy(&tri, &t.tris[12u * (size_t)k + 3u], 4);
        for (int v = 0; v < 3; v++) std::memcpy(&t.tris[12u * (size_t)k + 4u * v], &b4[4u * (size_t)idx[3u * tri + v]], 12);
    }
    const MeshDev sweep = mesh_dev(b4, vertex_count, idx, index_count, nullptr), stale = mesh_dev(b4, vertex_count, idx, index_count, &t);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < index_count; i++)
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min(lo[a], verts_b[3u * (size_t)idx[i] + a]);
            hi[a] = std::max(hi[a], verts_b[3u * (size_t)idx[i] + a]);
        }
    for (uint32_t r = 0; r < aimed; r++) {
        const double target[3] = {rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), rng.uniform(lo[2], hi[2])};
        const double o[3] = {0.5 * (lo[0] + hi[0]) + rng.uniform(-2, 2) * (hi[0] - lo[0] + 1.0), hi[1] + rng.uniform(0.5, 2.0) * (hi[1] - lo[1] + 1.0),
                             0.5 * (lo[2] + hi[2]) + rng.uniform(-2, 2) * (hi[2] - lo[2] + 1.0)};
        double dir[3], l = 0.0;
        for (int a = 0; a < 3; a++) {
            dir[a] = target[a] - o[a];
            l += dir[a] * dir[a];
        }
        const V3 ov{(float)o[0], (float)o[1], (float)o[2]};
        const V3 dv{(float)(dir[0] / std::sqrt(l)), (float)(dir[1] / std::sqrt(l)), (float)(dir[2] / std::sqrt(l))};
        Stack stk{};
        float t0 = 0.0f, t1 = 0.0f, ta = 0.0f;
        V3 n0{0, 0, 0}, n1{0, 0, 0}, na{0, 0, 0};
        const bool h0 = mesh_sweep(sweep, ov, 1e-4f, dv, 1e30f, t0, n0);
        const bool h1 = mesh_closest(stale, ov, 1e-4f, dv, 1e30f, t1, n1, stk);
        const bool a1 = mesh_any(stale, ov, 1e-4f, dv, 1e30f, ta, na, stk);
        out[0] += h0 != h1 || (h0 && (f_bits(t0) != f_bits(t1) || f_bits(n0.x) != f_bits(n1.x) || f_bits(n0.y) != f_bits(n1.y) || f_bits(n0.z) != f_bits(n1.z)));
        out[1] += a1 != h0;
        out[2] += h0;
    }
    return 0;
}
