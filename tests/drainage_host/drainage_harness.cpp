// tests/drainage_host/drainage_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_drainage_host.py compiles it).
// The drainage kernels' lane bodies (f3d_drainage.h: what k_drain_direction, k_drain_jump, k_drain_add, k_drain_write,
// k_stream_count and k_stream_emit run per lane) on the host over whole 64-lane waves: wave t owns tile t of 8 x 8 samples in
// the direction pass; a round is a Jacobi sweep -- every lane's jump into the second pair of planes, then every live lane's
// add as a plain sum --, repeated while the sweep before counted a live sample; the stream passes give wave b samples
// [64 b, 64 b + 64) of the region, a plain loop is the exclusive scan.  The ballots, the atomics and the scan are written as
// loops, everything else is the kernels' own code.
// With -DDRAINAGE_DRIVER (or -DDRAINAGE_HOST_DRIVER) the file is a stand-alone program (its own main) over synthetic DEMs, for
// a sanitizer build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../../forge3d_amd/csrc/f3d_drainage.h"

namespace {

struct Routed {
    std::vector<uint8_t> code;
    std::vector<uint32_t> q, s, q_next, s_next, depth;
    uint32_t sinks, rounds, longest;
};

// the direction pass and the rounds; P.q and P.s are the final planes
void route(const TerrainDev &T, DrainParams &P, Routed &R) {
    P.terrain = T;
    P.w = T.cell_w + 1u, P.h = T.cell_h + 1u;
    P.diag = drain_diag(T.spacing_x, T.spacing_z);
    const size_t n = (size_t)P.w * P.h;
    R.code.assign(n, 0xEEu);
    for (auto *plane : {&R.q, &R.s, &R.q_next, &R.s_next, &R.depth}) plane->assign(n, 0xEEEEEEEEu);
    std::vector<uint32_t> live(kDrainMaxRounds + 1u, 0u);  // (the device's slotted counters, summed: plain words here)
    P.code = R.code.data(), P.q = R.q.data(), P.s = R.s.data(), P.q_next = R.q_next.data(), P.s_next = R.s_next.data(), P.depth = R.depth.data();
    P.counters = nullptr;  // (the lane bodies never touch them)
    R.sinks = R.longest = 0u;
    for (uint32_t tile = 0; tile < drain_tiles(P.w, P.h); tile++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i, j;
            if (drain_tile_sample(P.w, P.h, tile, lane, i, j) && drain_lane_direction(P, i, j)) R.sinks++;
        }
    R.rounds = 0u;
    live[0] = (uint32_t)(n - R.sinks);
    for (uint32_t k = 0u; live[k] != 0u; k++) {
        P.round = k;
        for (uint32_t v = 0; v < n; v++) {
            uint32_t depth;
            if (drain_lane_jump(P, v, depth)) live[k + 1u]++;
            if (depth > R.longest) R.longest = depth;
        }
        for (uint32_t v = 0; v < n; v++) {
            uint32_t target, amount;
            if (drain_lane_add(P, v, target, amount)) P.s_next[target] += amount;
        }
        std::swap(P.q, P.q_next);
        std::swap(P.s, P.s_next);
        R.rounds++;
    }
}

void run_drainage(const TerrainDev &T, const uint32_t region[4], uint8_t *direction, uint32_t *accumulation, uint32_t *basin, uint32_t *stats) {
    DrainParams P{};
    Routed R;
    route(T, P, R);
    stats[0] = R.sinks, stats[1] = R.rounds, stats[2] = R.longest;
    P.row0 = region[0], P.col0 = region[1], P.rows = region[2], P.cols = region[3];
    P.out_direction = direction, P.out_accumulation = accumulation, P.out_basin = basin;
    for (uint32_t n = 0; n < P.rows * P.cols; n++) drain_lane_write(P, n);
}

uint64_t run_streams(const TerrainDev &T, const uint32_t region[4], uint32_t threshold, uint64_t capacity, float *segments, uint32_t *accumulation,
                     PaintPrim *prims, const float *rgba) {
    DrainParams P{};
    Routed R;
    route(T, P, R);
    P.row0 = region[0], P.col0 = region[1], P.rows = region[2], P.cols = region[3];
    P.threshold = threshold;
    const uint32_t waves = stream_waves(P.rows, P.cols);
    std::vector<uint64_t> totals((size_t)waves + 1u, 0u), offsets((size_t)waves + 1u, 0u);
    for (uint32_t b = 0; b <= waves; b++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i, j, code, acc;
            if (stream_lane(P, b * 64u + lane, i, j, code, acc)) totals[b]++;
        }
    for (uint32_t b = 0; b < waves; b++) offsets[b + 1u] = offsets[b] + totals[b];
    if (rgba)
        for (int c = 0; c < 4; c++) P.rgba[c] = rgba[c];
    for (uint32_t b = 0; b < waves; b++) {
        uint64_t at = offsets[b];
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i, j, code, acc;
            if (!stream_lane(P, b * 64u + lane, i, j, code, acc)) continue;
            const uint64_t here = at++;
            if (here >= capacity) continue;
            float ax, az, bx, bz;
            stream_segment(T, i, j, code, ax, az, bx, bz);
            if (prims) prims[here] = contour_prim(P.rgba, ax, az, bx, bz);
            if (segments) segments[4u * here] = ax, segments[4u * here + 1u] = az, segments[4u * here + 2u] = bx, segments[4u * here + 3u] = bz;
            if (accumulation) accumulation[here] = acc;
        }
    }
    return offsets[waves];
}

}  // namespace

// info[0..3] = terrain origin x, origin z, spacing x, spacing z; dims[0..2] = cell_w, cell_h, mip_count
extern "C" void *drain_scene_create(const f3d_terrain_ref_desc *d, float *info, uint32_t *dims) {
    HostScene *S = new HostScene();
    try {
        setup(*S, d, 1, 0u, 0u);
    } catch (const Failure &) {
        delete S;
        return nullptr;
    }
    const TerrainDev &T = S->P.terrain;
    if (info) info[0] = T.origin_x, info[1] = T.origin_z, info[2] = T.spacing_x, info[3] = T.spacing_z;
    if (dims) dims[0] = T.cell_w, dims[1] = T.cell_h, dims[2] = T.mip_count;
    return S;
}

extern "C" void drain_scene_destroy(void *scene) { delete (HostScene *)scene; }

// the session's heights: sample (i, j) as the leaf table holds it
extern "C" void drain_heights(void *scene, float *out) {
    const TerrainDev &T = ((const HostScene *)scene)->P.terrain;
    for (uint32_t j = 0; j <= T.cell_h; j++)
        for (uint32_t i = 0; i <= T.cell_w; i++) out[(size_t)j * (T.cell_w + 1u) + i] = lattice_height(T, i, j);
}

// One call as f3d_session_drainage answers it: region = {row0, col0, rows, cols}; stats = {sinks, rounds, longest}.
extern "C" void drain_run(void *scene, const uint32_t *region, uint8_t *direction, uint32_t *accumulation, uint32_t *basin, uint32_t *stats) {
    run_drainage(((const HostScene *)scene)->P.terrain, region, direction, accumulation, basin, stats);
}

// One call as f3d_session_streams answers it (prims null) or as f3d_session_paint_streams fills the paint buffer (prims: 20
// words a record).  Returns the total.
extern "C" uint64_t stream_run(void *scene, const uint32_t *region, uint32_t threshold, uint64_t capacity, float *segments, uint32_t *accumulation,
                               void *prims, const float *rgba) {
    return run_streams(((const HostScene *)scene)->P.terrain, region, threshold, capacity, segments, accumulation, (PaintPrim *)prims, rgba);
}

extern "C" uint32_t drain_desc_size(int which) {
    return which == 0 ? (uint32_t)sizeof(f3d_session_drainage_desc)
                      : (which == 1 ? (uint32_t)sizeof(f3d_session_streams_desc) : (uint32_t)sizeof(f3d_session_paint_streams_desc));
}

#if defined(DRAINAGE_DRIVER) || defined(DRAINAGE_HOST_DRIVER)
// A 65 x 63, a 10 x 9, a 5 x 3 and a 2 x 2 synthetic DEM, and a flat one; whole and unaligned regions; thresholds 1, 3 and one
// above every accumulation; a capacity below the total; both output forms.  Prints one line; exit status 0 when the sinks'
// accumulations sum to w * h, every basin is a sink, the region is the whole DEM's window and the forms agree.
int main() {
    unsigned long long segments_total = 0ull, bad = 0ull, rounds_total = 0ull;
    const uint32_t shapes[5][2] = {{65u, 63u}, {10u, 9u}, {5u, 3u}, {2u, 2u}, {9u, 9u}};
    for (int c = 0; c < 5; c++) {
        const uint32_t w = shapes[c][0], h = shapes[c][1];
        std::vector<float> dem((size_t)w * h);
        for (uint32_t z = 0; z < h; z++)
            for (uint32_t x = 0; x < w; x++)
                dem[(size_t)z * w + x] = c == 4 ? 1.0f : 3.0f * std::sin(0.37f * (float)x) * std::cos(0.23f * (float)z) + 0.05f * (float)((x * 7u + z * 13u) % 11u);
        HostTables t = build_tables_host(dem.data(), w, h, 20.0f);
        TerrainDev T{};
        t.attach(T);
        T.spacing_x = 30.0f;
        T.spacing_z = 25.0f;
        T.origin_x = -0.5f * ((float)w - 1.0f) * T.spacing_x;
        T.origin_z = -0.5f * ((float)h - 1.0f) * T.spacing_z;
        const uint32_t whole[4] = {0u, 0u, h, w};
        const size_t n = (size_t)w * h;
        std::vector<uint8_t> dir(n);
        std::vector<uint32_t> acc(n), basin(n);
        uint32_t stats[3];
        run_drainage(T, whole, dir.data(), acc.data(), basin.data(), stats);
        unsigned long long sum = 0ull, sinks = 0ull;
        for (size_t v = 0; v < n; v++) {
            if (dir[v] == kDrainSink) sum += acc[v], sinks++, bad += basin[v] != v ? 1ull : 0ull;
            bad += (basin[v] >= n || dir[basin[v]] != kDrainSink) ? 1ull : 0ull;
        }
        bad += (sum != n || sinks != stats[0]) ? 1ull : 0ull;
        bad += (c == 4 && (stats[1] != 0u || stats[2] != 0u || sinks != n)) ? 1ull : 0ull;
        rounds_total += stats[1];
        const uint32_t part[4] = {h > 3u ? 1u : 0u, w > 4u ? 2u : 0u, h > 3u ? h - 3u : h, w > 4u ? w - 4u : w};
        std::vector<uint8_t> pdir((size_t)part[2] * part[3]);
        std::vector<uint32_t> pacc(pdir.size());
        uint32_t pstats[3];
        run_drainage(T, part, pdir.data(), pacc.data(), nullptr, pstats);
        for (uint32_t r = 0; r < part[2]; r++)
            for (uint32_t q = 0; q < part[3]; q++) {
                const size_t v = (size_t)(part[0] + r) * w + part[1] + q, m = (size_t)r * part[3] + q;
                bad += (pdir[m] != dir[v] || pacc[m] != acc[v]) ? 1ull : 0ull;
            }
        const float rgba[4] = {0.1f, 0.3f, 0.8f, 1.0f};
        for (uint32_t threshold : {1u, 3u, (uint32_t)n + 1u})
            for (const uint32_t *region : {whole, part}) {
                const uint64_t total = run_streams(T, region, threshold, 0u, nullptr, nullptr, nullptr, nullptr);
                std::vector<float> a((size_t)total * 4u + 4u, 77.0f);
                std::vector<uint32_t> ia((size_t)total + 1u, 77u);
                std::vector<PaintPrim> prims((size_t)total / 2u + 1u);
                bad += run_streams(T, region, threshold, total, a.data(), ia.data(), nullptr, nullptr) != total;
                (void)run_streams(T, region, threshold, total / 2u, nullptr, nullptr, prims.data(), rgba);
                for (size_t q = 0; q < (size_t)total * 4u; q++) bad += !std::isfinite(a[q]) ? 1ull : 0ull;
                for (size_t q = 0; q < (size_t)total; q++) bad += ia[q] < threshold ? 1ull : 0ull;
                for (size_t q = 0; q < (size_t)(total / 2u); q++) bad += (prims[q].v[0] != a[4u * q] || prims[q].v[5] != a[4u * q + 3u]) ? 1ull : 0ull;
                bad += (a[(size_t)total * 4u] != 77.0f || ia[(size_t)total] != 77u) ? 1ull : 0ull;
                bad += (threshold > n && total != 0u) ? 1ull : 0ull;
                segments_total += total;
            }
    }
    printf("drainage driver: %llu segments, %llu rounds, disagreements: %llu\n", segments_total, rounds_total, bad);
    return bad == 0ull ? 0 : 1;
}
#endif
