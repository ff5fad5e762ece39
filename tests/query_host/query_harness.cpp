// tests/query_host/query_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_query_host.py compiles it).
// The ray queries' lane body (f3d_query.h query_lane, what k_query runs per lane) on the host over whole 64-lane waves:
// the lanes are the emulator's fibers, the votes of the marches are exchanged in lockstep, a lane whose ray is bad leaves
// the wave without having voted.  The scene is the emulator's (host-built tables and mesh BVHs from the product's builders).
// The pending type is the device's in what matters to the answers' provenance: closest-hit rays are not shared
// (LdsPending::kShareClosest is false), so the march hands out the hit cell.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../../forge3d_amd/csrc/f3d_query.h"

namespace {
struct QueryPending : WavePending {
    static constexpr bool kShareClosest = false;
};
}  // namespace

// mesh_form: 0 the reference's sweep, 1 the threaded binary walk, 2 four children wide.
// info[0..3] = terrain origin x, origin z, inv_two_r_prime, curvature_enabled (what the oracle's ray batch wants).
extern "C" void *query_scene_create(const f3d_terrain_ref_desc *d, int32_t mesh_form, float *info) {
    HostScene *S = new HostScene();
    try {
        setup(*S, d, mesh_form == 2 ? 2 : 1, 0u, 0u);
    } catch (const Failure &) {
        delete S;
        return nullptr;
    }
    if (mesh_form == 0) {
        S->P.mesh.bvh_nodes = nullptr;
        S->P.mesh.bvh4_nodes = nullptr;
        S->P.mesh.bvh_tris = nullptr;
    }
    if (info) {
        info[0] = S->P.terrain.origin_x;
        info[1] = S->P.terrain.origin_z;
        info[2] = S->P.terrain.inv_two_r_prime;
        info[3] = (float)S->P.terrain.curvature_enabled;
    }
    return S;
}

extern "C" void query_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One batch as f3d_session_query answers it (flags: 1 TERRAIN_ONLY, 2 CURVED).  marches (count words, may be null): how
// many terrain marches lane i entered.
extern "C" int query_run(void *scene, uint32_t mode, uint32_t flags, uint32_t count, const void *rays, uint32_t *kind, float *t,
                         float *normal, float *position, uint32_t *primitive, float *direction, uint32_t *marches) {
    const HostScene &S = *(const HostScene *)scene;
    QueryParams Q{};
    Q.frame = S.P;
    if (flags & 1u) Q.frame.mesh.traversal_mode = 3u;
    Q.mode = mode;
    Q.curved = (flags & 2u) ? 1u : 0u;
    Q.count = count;
    if (mode == kQueryPixels) Q.pixels = (const uint2 *)rays;
    else Q.rays = (const float4 *)rays;
    Q.kind = kind;
    Q.t = t;
    Q.normal = normal;
    Q.position = position;
    Q.primitive = primitive;
    Q.direction = direction;
    const long waves = ((long)count + 63) / 64;
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++) {
        Wave wave;
        const uint32_t first = (uint32_t)wv * 64u, n = count - first < 64u ? count - first : 64u;
        const uint64_t mask = n == 64u ? ~0ull : ((1ull << n) - 1ull);
        wave.run(mask, [&](int lane) {
            QueryPending pend;
            pend.wave = &wave;
            pend.me = lane;
            std::vector<RayLog> log;
            pend.log = &log;
            query_lane(Q, first + (uint32_t)lane, pend);
            if (marches) marches[first + (uint32_t)lane] = (uint32_t)log.size();
        });
    }
    return 0;
}
