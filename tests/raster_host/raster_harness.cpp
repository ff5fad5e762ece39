// tests/raster_host/raster_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_raster_host.py compiles it).
// The visibility rasters' lane body (f3d_raster.h raster_origin / raster_visible, what k_raster runs per lane) on the host
// over whole 64-lane waves: wave b owns samples [64 b, 64 b + 64) of the region, as on the device.  The lanes are the
// emulator's fibers and the marches' votes are exchanged in lockstep; a wave is run once per target, and a lane that is cut
// off by the distance limit or whose ray is refused leaves that wave without having voted -- the region k_raster's lanes
// skip with their EXEC bit off.  The mask word is put together from the lanes' answers as the device's ballot does it.
// The loop over the targets below is this harness's own, NOT k_raster's: here every target gets a fresh pending context and a
// wave of its own, on the device one context and its LDS rows serve all targets, a lane may march for target k and sit out
// target k + 1, and the ballot after each target is the mask word.  That loop is covered by tests/test_gpu_raster.py alone
// (K = 3 with the distance-limited and the on-sample observer between marching targets); what runs here is the lane body.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../../forge3d_amd/csrc/f3d_raster.h"

namespace {
struct RasterPending : WavePending {
    static constexpr bool kShareClosest = false;
};
}  // namespace

// mesh_form: 0 the reference's sweep, 1 the threaded binary walk, 2 four children wide.
// info[0..8]: scene_create's nine (tests/emul/host_scene.h)
extern "C" void *raster_scene_create(const f3d_terrain_ref_desc *d, int32_t mesh_form, float *info) {
    HostScene *S = scene_create(d, mesh_form, info, 9u);
    if (S && mesh_form == 0) {
        S->P.mesh.bvh_nodes = nullptr;
        S->P.mesh.bvh4_nodes = nullptr;
        S->P.mesh.bvh_tris = nullptr;
    }
    return S;
}

extern "C" void raster_scene_destroy(void *scene) { delete (HostScene *)scene; }

// One raster as f3d_session_raster's device form answers it (flags: 1 TERRAIN_ONLY, 2 CURVED, 16 SESSION_SUN; targets null
// with SESSION_SUN).  marches (target_count x rows * cols words, may be null): how many terrain marches the lane of sample n
// entered for target k.  origins (rows * cols x 3, may be null): the lifted lattice points.
extern "C" int raster_run(void *scene, uint32_t mode, uint32_t flags, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, float lift,
                          uint32_t target_count, const float *targets, uint64_t *masks, uint32_t *count, uint32_t *marches, float *origins) {
    const HostScene &S = *(const HostScene *)scene;
    RasterParams R{};
    R.frame = S.P;
    if (flags & 1u) R.frame.mesh.traversal_mode = 3u;
    R.mode = mode;
    R.curved = (flags & 2u) ? 1u : 0u;
    R.row0 = row0;
    R.col0 = col0;
    R.rows = rows;
    R.cols = cols;
    R.lift = lift;
    R.target_count = (flags & 16u) ? 1u : target_count;
    R.targets = (flags & 16u) ? nullptr : (const float4 *)targets;
    const uint32_t total = rows * cols;
    const long waves = ((long)total + 63) / 64;
    const size_t words = (size_t)waves;
#pragma omp parallel for schedule(dynamic, 1)
    for (long wv = 0; wv < waves; wv++) {
        Wave wave;
        const uint32_t first = (uint32_t)wv * 64u, n = total - first < 64u ? total - first : 64u;
        const uint64_t lanes = n == 64u ? ~0ull : ((1ull << n) - 1ull);
        V3 o[64];
        uint32_t seen[64] = {};
        for (uint32_t l = 0; l < n; l++) {
            o[l] = raster_origin(R, first + l);
            store_point(origins, first + l, o[l]);
        }
        for (uint32_t k = 0; k < R.target_count; k++) {
            const float4 target = R.targets ? R.targets[k] : float4{R.frame.light.wi.x, R.frame.light.wi.y, R.frame.light.wi.z, 0.0f};
            uint64_t word = 0;
            wave.run(lanes, [&](int lane) {
                RasterPending pend;
                pend.wave = &wave;
                pend.me = lane;
                std::vector<RayLog> log;
                pend.log = &log;
                const bool visible = raster_visible(R, o[lane], target, pend);
                if (visible) word |= 1ull << lane;  // (fibers of one thread: no race)
                if (marches) marches[(size_t)k * total + first + (uint32_t)lane] = (uint32_t)log.size();
            });
            if (masks) masks[(size_t)k * words + (size_t)wv] = word;
            for (uint32_t l = 0; l < n; l++) seen[l] += (uint32_t)((word >> l) & 1ull);
        }
        if (count)
            for (uint32_t l = 0; l < n; l++) count[first + l] = seen[l];
    }
    return 0;
}

extern "C" uint32_t raster_desc_size() { return (uint32_t)sizeof(f3d_session_raster_desc); }
