// tests/rearm_host/rearm_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_rearm_host.py compiles it).
// The re-arm pass's pixel body (f3d_shade.h rearm_certificate, what k_rearm runs per pixel) on the host against the
// G-buffer pass (gbuffer_pixel, what k_gbuffer runs): a G-buffer made under sun A, re-armed for sun B, must hold the
// sun-ray certificates that the G-buffer pass writes under sun B, bit for bit.  The product's headers through the
// emulator's scene set-up (host-built tables and mesh BVHs), one "lane" at a time.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"

namespace {
void gbuffer(const FrameParams &P, std::vector<float4> &gbuf, std::vector<float> &dep, std::vector<float2> &sun) {
    const uint32_t W = P.cam.width, H = P.row_end - P.row_begin;
    gbuf.assign((size_t)W * H, float4{0.0f, 0.0f, 0.0f, 0.0f});
    dep.assign((size_t)W * H, 0.0f);
    sun.assign((size_t)W * H, float2{0.0f, 0.0f});
    FrameParams Q = P;
    Q.sun_clear = sun.data();
    Q.primary_start = nullptr;
#pragma omp parallel for schedule(dynamic, 4)
    for (long y = 0; y < (long)H; y++) {
        ArrayPending pend;
        for (uint32_t x = 0; x < W; x++) gbuffer_pixel(Q, x, (uint32_t)y, gbuf.data(), dep.data(), pend);
    }
}
}  // namespace

// sun A -> G-buffer; re-armed under sun B; compared with the G-buffer pass under sun B.
// out[0] pixels, [1] hit pixels, [2] certificates that differ, [3] G-buffer / depth words that differ between the two
// G-buffer passes (the camera is the same: must be 0), [4] hit pixels whose sun-B certificate is finite (coverage).
// Returns 0, or 1 when a descriptor is refused.
extern "C" int rearm_check(const f3d_terrain_ref_desc *a, const f3d_terrain_ref_desc *b, int32_t mesh_form, uint64_t *out) {
    try {
        HostScene SA, SB;
        setup(SA, a, mesh_form, 0u, 0u);
        setup(SB, b, mesh_form, 0u, 0u);
        std::vector<float4> gbuf_a, gbuf_b;
        std::vector<float> dep_a, dep_b;
        std::vector<float2> sun_a, sun_b;
        gbuffer(SA.P, gbuf_a, dep_a, sun_a);
        gbuffer(SB.P, gbuf_b, dep_b, sun_b);
        // the re-arm: sun B's uniforms over sun A's resident G-buffer and certificates
        FrameParams R = SB.P;
        R.sun_clear = sun_a.data();
        const uint32_t W = R.cam.width, H = R.row_end - R.row_begin;
#pragma omp parallel for schedule(dynamic, 4)
        for (long y = 0; y < (long)H; y++)
            for (uint32_t x = 0; x < W; x++) rearm_certificate(R, x, (uint32_t)y, gbuf_a.data(), dep_a.data());
        uint64_t hits = 0, bad = 0, gbad = 0, finite = 0;
        for (size_t i = 0; i < (size_t)W * H; i++) {
            if (memcmp(&sun_a[i], &sun_b[i], sizeof(float2)) != 0) bad++;
            if (memcmp(&gbuf_a[i], &gbuf_b[i], sizeof(float4)) != 0 || memcmp(&dep_a[i], &dep_b[i], sizeof(float)) != 0) gbad++;
            if (gbuf_b[i].w != 0.0f) {
                hits++;
                if (sun_b[i].x < 1e30f) finite++;
            }
        }
        out[0] = (uint64_t)W * H;
        out[1] = hits;
        out[2] = bad;
        out[3] = gbad;
        out[4] = finite;
        return 0;
    } catch (const Failure &) {
        return 1;
    }
}
