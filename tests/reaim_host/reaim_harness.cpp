// tests/reaim_host/reaim_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_reaim_host.py compiles it).
// The re-aim pass's pixel body (f3d_shade.h reaim_pixel, what k_reaim runs per pixel) on the host against the G-buffer
// pass (gbuffer_pixel, what k_gbuffer runs): a strip's state made under camera A and sun A -- G-buffer, depth, primary-ray
// and sun-ray certificates -- with every per-render array filled with a byte pattern, re-aimed to camera B and sun B, must
// hold bit for bit what the G-buffer pass writes in a fresh scene under B, and cleared arrays as a create leaves them.
// The product's headers through the emulator's scene set-up (host-built tables and mesh BVHs), one "lane" at a time.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"

namespace {
// what the G-buffer pass writes for a strip
struct GBuffer {
    std::vector<float4> n;
    std::vector<float> depth;
    std::vector<float2> sun;
    std::vector<uint2> start;
};

void gbuffer(const FrameParams &P, GBuffer &G) {
    const uint32_t W = P.cam.width, rows = P.row_end - P.row_begin;
    const size_t px = (size_t)W * rows;
    G.n.assign(px, float4{0.0f, 0.0f, 0.0f, 0.0f});
    G.depth.assign(px, 0.0f);
    G.sun.assign(px, float2{0.0f, 0.0f});
    G.start.assign(px, uint2{0u, 0u});
    FrameParams Q = P;
    Q.sun_clear = G.sun.data();
    Q.primary_start = G.start.data();
#pragma omp parallel for schedule(dynamic, 4)
    for (long y = P.row_begin; y < (long)P.row_end; y++) {
        ArrayPending pend;
        for (uint32_t x = 0; x < W; x++) gbuffer_pixel(Q, x, (uint32_t)y, G.n.data(), G.depth.data(), pend);
    }
}

template <class T>
uint64_t differing(const std::vector<T> &a, const std::vector<T> &b) {
    uint64_t n = a.size() == b.size() ? 0u : 1u;
    for (size_t i = 0; i < a.size() && i < b.size(); i++) n += memcmp(&a[i], &b[i], sizeof(T)) != 0;
    return n;
}
template <class T>
uint64_t nonzero_bytes(const std::vector<T> &a) {
    uint64_t n = 0;
    const uint8_t *p = (const uint8_t *)a.data();
    for (size_t i = 0; i < a.size() * sizeof(T); i++) n += p[i] != 0u;
    return n;
}
}  // namespace

// State under (camera A, sun A), every per-render array filled with `pattern`; re-aimed to b; compared with a fresh
// G-buffer pass under b.  rows [row_begin, row_end) of the image (0, 0: all).  trace: frames in flight are on (the head
// records hold the first prediction instead of zeros); heads = 0: the session has no head records.
// out[0] pixels, [1] pixels hit under b, [2] G-buffer records that differ, [3] depth words, [4] sun certificates,
// [5] primary-ray certificates, [6] non-zero bytes left in the cleared arrays (accumulation, Welford, both reservoir
// buffers with halo rows, tile costs, stats, retrace counters), [7] head records that differ from a create's, [8] sky
// pixels under b whose depth is not the quiet NaN 0x7fc00000, [9] G-buffer records that differ between a and b (how much
// the camera changed), [10] head records with the prediction bit set.
// Returns 0, or 1 when a descriptor is refused.
extern "C" int reaim_check(const f3d_terrain_ref_desc *a, const f3d_terrain_ref_desc *b, int32_t mesh_form, uint32_t row_begin,
                           uint32_t row_end, int32_t trace, int32_t heads, uint32_t pattern, uint64_t *out) {
    try {
        HostScene SA, SB;
        setup(SA, a, mesh_form, row_begin, row_end);
        setup(SB, b, mesh_form, row_begin, row_end);
        GBuffer GA, GB;
        gbuffer(SA.P, GA);
        gbuffer(SB.P, GB);
        const std::vector<float4> a_n = GA.n;
        const uint32_t W = SB.P.cam.width, rows = SB.P.row_end - SB.P.row_begin;
        const size_t px = (size_t)W * rows, res_n = (size_t)(rows + 2u * kHaloRows) * W;
        const uint32_t tiles = ((W + 7u) / 8u) * ((rows + 7u) / 8u);
        const uint8_t fill = (uint8_t)pattern;
        std::vector<float4> accum(px);
        std::vector<float> m2(px);
        std::vector<PackedReservoir> res[2] = {std::vector<PackedReservoir>(res_n), std::vector<PackedReservoir>(res_n)};
        std::vector<uint2> head(heads ? px : 0u);
        std::vector<uint32_t> tile_cost(tiles), stats(4), fix_count(4);
        std::vector<float4> records(1);
        memset(accum.data(), fill, px * sizeof(float4));
        memset(m2.data(), fill, px * sizeof(float));
        for (auto &r : res) memset((void *)r.data(), fill, res_n * sizeof(PackedReservoir));
        if (heads) memset(head.data(), fill, px * sizeof(uint2));
        memset(tile_cost.data(), fill, tiles * sizeof(uint32_t));
        memset(stats.data(), fill, 4 * sizeof(uint32_t));
        memset(fix_count.data(), fill, 4 * sizeof(uint32_t));

        // the re-aim: b's uniforms over a's resident state
        RearmParams R{};
        R.frame = SB.P;
        R.frame.gbuffer_n = GA.n.data();
        R.frame.sun_clear = GA.sun.data();
        R.frame.primary_start = GA.start.data();
        R.frame.accum_mean = accum.data();
        R.frame.welford_m2 = m2.data();
        R.frame.head = heads ? head.data() : nullptr;
        R.frame.trace = trace ? records.data() : nullptr;
        R.frame.stats = stats.data();
        R.frame.fix_count = trace ? fix_count.data() : nullptr;
        R.gbuffer_n = GA.n.data();
        R.depth = GA.depth.data();
        R.res[0] = res[0].data();
        R.res[1] = res[1].data();
        R.tile_cost = tile_cost.data();
        R.tiles = tiles;
        if (!trace) memset(fix_count.data(), 0, 4 * sizeof(uint32_t));  // (a session without frames in flight has none)
#pragma omp parallel for schedule(dynamic, 4)
        for (long y = R.frame.row_begin; y < (long)R.frame.row_end; y++) {
            ArrayPending pend;
            for (uint32_t x = 0; x < W; x++) reaim_pixel(R, x, (uint32_t)y, pend);
        }

        uint64_t hits = 0, sky_bad = 0, head_bad = 0, head_set = 0;
        for (size_t i = 0; i < px; i++) {
            if (GB.n[i].w != 0.0f) hits++;
            else if (f_bits(GA.depth[i]) != 0x7fc00000u) sky_bad++;
            if (heads) {
                uint2 want = uint2{0u, 0u};
                if (trace) want = uint2{0u, (GB.n[i].w != 0.0f && dot(V3{GB.n[i].x, GB.n[i].y, GB.n[i].z}, SB.P.light.wi) > 0.0f) ? 1u : 0u};
                head_bad += memcmp(&head[i], &want, sizeof(uint2)) != 0;
                head_set += head[i].y != 0u;
            }
        }
        out[0] = px;
        out[1] = hits;
        out[2] = differing(GA.n, GB.n);
        out[3] = differing(GA.depth, GB.depth);
        out[4] = differing(GA.sun, GB.sun);
        out[5] = differing(GA.start, GB.start);
        out[6] = nonzero_bytes(accum) + nonzero_bytes(m2) + nonzero_bytes(res[0]) + nonzero_bytes(res[1]) + nonzero_bytes(tile_cost) +
                 nonzero_bytes(stats) + nonzero_bytes(fix_count);
        out[7] = head_bad;
        out[8] = sky_bad;
        out[9] = differing(a_n, GB.n);
        out[10] = head_set;
        return 0;
    } catch (const Failure &) {
        return 1;
    }
}
