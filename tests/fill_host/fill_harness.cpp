// tests/fill_host/fill_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/fill_cases.py compiles it).
// The fill kernels' bodies (f3d_fill.h: what k_fill_init, k_flat_init, k_fill_direction, k_fill_stats and k_fill_write run per
// lane, and what a workgroup of k_fill_relax / k_flat_relax runs per tile) on the host.  A tile's threads run one after the
// other in every phase -- load, sweeps until one lowers nothing, store --, which is one of the schedules the device may take;
// the tiles of a round run in index order (seed 0) or in an order shuffled by the seed, so that halo reads see the round's
// new values in two different patterns.  The tile body is instantiated at the device's edge and at an edge of 8.  The atomics,
// the ballots and the scan are loops; the doubling rounds and the stream passes are tests/drainage_host's loops over
// f3d_drainage.h's lanes, behind fill_lane_direction (fill on) or drain_lane_direction (fill off).
// With -DFILL_HOST_DRIVER the file is a stand-alone program (its own main) over the 35 x 35 walled serpentine, for a sanitizer
// build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../../forge3d_amd/csrc/f3d_fill.h"

#include <numeric>

namespace {

struct Filled {
    std::vector<float> z, W;
    std::vector<uint32_t> T, dirty[2];
    uint32_t rounds[2], filled_samples, largest;
};

// the tiles of round r in the order of the seed
std::vector<uint32_t> tile_order(uint32_t tiles, uint32_t seed, uint32_t r) {
    std::vector<uint32_t> order(tiles);
    std::iota(order.begin(), order.end(), 0u);
    if (seed == 0u) return order;
    uint64_t state = 0x9E3779B97F4A7C15ull * (seed + 1u) + r;
    for (uint32_t n = tiles; n > 1u; n--) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(order[n - 1u], order[(uint32_t)((state >> 33) % n)]);
    }
    return order;
}

// one round of k_fill_relax / k_flat_relax: returns the tiles marked for the next
template <uint32_t E, class Rule>
uint32_t relax_round(FillParams &F, uint32_t seed) {
    typedef FillTileBody<E, Rule> Body;
    std::vector<typename Rule::A> a(Body::kWords);
    std::vector<typename Rule::B> b(Body::kWords);
    const uint32_t now = F.round & 1u, next = now ^ 1u;
    uint32_t marked = 0u;
    for (uint32_t tile : tile_order(fill_tiles(F.w, F.h, E), seed, F.round)) {
        if (F.dirty[now][tile] == 0u) continue;
        F.dirty[now][tile] = 0u;
        for (uint32_t t = 0; t < Body::kThreads; t++) Body::load(F, tile, t, a.data(), b.data());
        for (bool changed = true; changed;) {
            changed = false;
            for (uint32_t t = 0; t < Body::kThreads; t++) changed |= Body::sweep(t, a.data(), b.data());
        }
        uint32_t touched = 0u;
        for (uint32_t t = 0; t < Body::kThreads; t++) touched |= Body::store(F, tile, t, b.data());
        for (uint32_t k = 0; k < 8u; k++) {
            uint32_t other;
            if (((touched >> k) & 1u) != 0u && Body::neighbour(F, tile, k, other) && F.dirty[next][other] == 0u) F.dirty[next][other] = 1u, marked++;
        }
    }
    return marked;
}

template <uint32_t E>
void fill_passes(const TerrainDev &T, FillParams &F, Filled &R, uint32_t seed) {
    F.terrain = T;
    F.w = T.cell_w + 1u, F.h = T.cell_h + 1u;
    F.tile = E;
    const size_t n = (size_t)F.w * F.h;
    const uint32_t tiles = fill_tiles(F.w, F.h, E);
    R.z.assign(n, -7.0f), R.W.assign(n, -7.0f), R.T.assign(n, 0xEEEEEEEEu);
    R.dirty[0].assign(tiles, 0xEEu), R.dirty[1].assign(tiles, 0xEEu);
    F.z = R.z.data(), F.W = R.W.data(), F.T = R.T.data(), F.dirty[0] = R.dirty[0].data(), F.dirty[1] = R.dirty[1].data();
    F.counters = nullptr;  // (the bodies never touch them)
    for (uint32_t v = 0; v < n; v++) fill_lane_init(F, v);
    R.rounds[0] = R.rounds[1] = 0u;
    uint32_t marked = tiles;
    for (uint32_t r = 0u; marked != 0u; r++) F.round = r, marked = relax_round<E, FillRule>(F, seed), R.rounds[0]++;
    for (uint32_t v = 0; v < n; v++)
        if (flat_lane_init(F, v) && F.dirty[0][fill_tile_of(F, v)] == 0u) F.dirty[0][fill_tile_of(F, v)] = 1u, marked++;
    for (uint32_t r = 0u; marked != 0u; r++) F.round = r, marked = relax_round<E, FlatRule>(F, seed), R.rounds[1]++;
    R.filled_samples = R.largest = 0u;
    for (uint32_t v = 0; v < n; v++) {
        uint32_t flat;
        if (fill_lane_stats(F, v, flat)) R.filled_samples++;
        R.largest = std::max(R.largest, flat);
    }
}

void fill_passes(const TerrainDev &T, FillParams &F, Filled &R, uint32_t edge, uint32_t seed) {
    if (edge == 8u) fill_passes<8u>(T, F, R, seed);
    else fill_passes<kFillTile>(T, F, R, seed);
}

struct Routed {
    Filled filled;
    std::vector<uint8_t> code;
    std::vector<uint32_t> q, s, q_next, s_next, depth;
    uint32_t sinks, rounds, longest;
};

// the direction pass -- filled (edge != 0) or not -- and the doubling rounds; P.q and P.s are the final planes
void route(const TerrainDev &T, DrainParams &P, Routed &R, uint32_t edge, uint32_t seed) {
    P.terrain = T;
    P.w = T.cell_w + 1u, P.h = T.cell_h + 1u;
    P.diag = drain_diag(T.spacing_x, T.spacing_z);
    const size_t n = (size_t)P.w * P.h;
    if (edge != 0u) {
        FillParams F{};
        fill_passes(T, F, R.filled, edge, seed);
        P.fill_W = F.W, P.fill_T = F.T;
    }
    R.code.assign(n, 0xEEu);
    for (auto *plane : {&R.q, &R.s, &R.q_next, &R.s_next, &R.depth}) plane->assign(n, 0xEEEEEEEEu);
    P.code = R.code.data(), P.q = R.q.data(), P.s = R.s.data(), P.q_next = R.q_next.data(), P.s_next = R.s_next.data(), P.depth = R.depth.data();
    R.sinks = R.longest = R.rounds = 0u;
    for (uint32_t tile = 0; tile < drain_tiles(P.w, P.h); tile++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i, j;
            if (drain_tile_sample(P.w, P.h, tile, lane, i, j) && (edge != 0u ? fill_lane_direction(P, i, j) : drain_lane_direction(P, i, j))) R.sinks++;
        }
    for (uint32_t k = 0u, live = (uint32_t)(n - R.sinks); live != 0u; k++) {
        P.round = k;
        live = 0u;
        for (uint32_t v = 0; v < n; v++) {
            uint32_t depth;
            if (drain_lane_jump(P, v, depth)) live++;
            R.longest = std::max(R.longest, depth);
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

void run_fill(const TerrainDev &T, uint32_t edge, uint32_t seed, const uint32_t region[4], float *filled, float *depth, uint32_t *flat, uint32_t *stats) {
    FillParams F{};
    Filled R;
    fill_passes(T, F, R, edge, seed);
    if (stats) stats[0] = R.filled_samples, stats[1] = R.rounds[0], stats[2] = R.rounds[1], stats[3] = R.largest;
    F.row0 = region[0], F.col0 = region[1], F.rows = region[2], F.cols = region[3];
    F.out_filled = filled, F.out_depth = depth, F.out_flat = flat;
    for (uint32_t n = 0; n < F.rows * F.cols; n++) fill_lane_write(F, n);
}

void run_drainage(const TerrainDev &T, uint32_t edge, uint32_t seed, const uint32_t region[4], uint8_t *direction, uint32_t *accumulation, uint32_t *basin,
                  uint32_t *stats) {
    DrainParams P{};
    Routed R;
    route(T, P, R, edge, seed);
    stats[0] = R.sinks, stats[1] = R.rounds, stats[2] = R.longest;
    P.row0 = region[0], P.col0 = region[1], P.rows = region[2], P.cols = region[3];
    P.out_direction = direction, P.out_accumulation = accumulation, P.out_basin = basin;
    for (uint32_t n = 0; n < P.rows * P.cols; n++) drain_lane_write(P, n);
}

uint64_t run_streams(const TerrainDev &T, uint32_t edge, uint32_t seed, const uint32_t region[4], uint32_t threshold, uint64_t capacity, float *segments,
                     uint32_t *accumulation, PaintPrim *prims, const float *rgba) {
    DrainParams P{};
    Routed R;
    route(T, P, R, edge, seed);
    P.row0 = region[0], P.col0 = region[1], P.rows = region[2], P.cols = region[3];
    P.threshold = threshold;
    if (rgba)
        for (int c = 0; c < 4; c++) P.rgba[c] = rgba[c];
    uint64_t at = 0u;  // (count, scan and emit in one loop: the waves' totals in order are the running sum)
    for (uint32_t n = 0; n < stream_waves(P.rows, P.cols) * 64u; n++) {
        uint32_t i, j, code, acc;
        if (!stream_lane(P, n, i, j, code, acc)) continue;
        const uint64_t here = at++;
        if (here >= capacity) continue;
        float ax, az, bx, bz;
        stream_segment(T, i, j, code, ax, az, bx, bz);
        if (prims) prims[here] = contour_prim(P.rgba, ax, az, bx, bz);
        if (segments) segments[4u * here] = ax, segments[4u * here + 1u] = az, segments[4u * here + 2u] = bx, segments[4u * here + 3u] = bz;
        if (accumulation) accumulation[here] = acc;
    }
    return at;
}

}  // namespace

// info[0..3] = terrain origin x, origin z, spacing x, spacing z; dims[0..2] = cell_w, cell_h, mip_count
extern "C" void *fill_scene_create(const f3d_terrain_ref_desc *d, float *info, uint32_t *dims) {
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

extern "C" void fill_scene_destroy(void *scene) { delete (HostScene *)scene; }

extern "C" void fill_heights(void *scene, float *out) {
    const TerrainDev &T = ((const HostScene *)scene)->P.terrain;
    for (uint32_t j = 0; j <= T.cell_h; j++)
        for (uint32_t i = 0; i <= T.cell_w; i++) out[(size_t)j * (T.cell_w + 1u) + i] = lattice_height(T, i, j);
}

// One call as f3d_session_fill answers it, with the tile edge (8 or the device's) and the seed of the tile order:
// region = {row0, col0, rows, cols}; stats = {filled samples, fill rounds, flat rounds, largest T}.
extern "C" void fill_run(void *scene, uint32_t edge, uint32_t seed, const uint32_t *region, float *filled, float *depth, uint32_t *flat, uint32_t *stats) {
    run_fill(((const HostScene *)scene)->P.terrain, edge, seed, region, filled, depth, flat, stats);
}

// One call as f3d_session_drainage answers it; edge 0: without F3D_DRAINAGE_FILL.
extern "C" void fill_drain_run(void *scene, uint32_t edge, uint32_t seed, const uint32_t *region, uint8_t *direction, uint32_t *accumulation,
                               uint32_t *basin, uint32_t *stats) {
    run_drainage(((const HostScene *)scene)->P.terrain, edge, seed, region, direction, accumulation, basin, stats);
}

// One call as f3d_session_streams answers it (prims null) or as f3d_session_paint_streams fills the paint buffer.  Returns the total.
extern "C" uint64_t fill_stream_run(void *scene, uint32_t edge, uint32_t seed, const uint32_t *region, uint32_t threshold, uint64_t capacity,
                                    float *segments, uint32_t *accumulation, void *prims, const float *rgba) {
    return run_streams(((const HostScene *)scene)->P.terrain, edge, seed, region, threshold, capacity, segments, accumulation, (PaintPrim *)prims, rgba);
}

extern "C" uint32_t fill_desc_size() { return (uint32_t)sizeof(f3d_session_fill_desc); }
extern "C" uint32_t fill_tile_edge() { return kFillTile; }

#if defined(FILL_HOST_DRIVER)
// The 35 x 35 walled serpentine (tests/fill_cases.py: a channel that ascends to its end inside a frame with one gap), both
// edges and two tile orders.  Prints one line; exit status 0 when the four runs agree in every plane, W >= z, every sink is an
// outlet, the sinks' accumulations sum to w * h and the known answers hold.
int main() {
    const uint32_t n = 33u, w = n + 2u;
    std::vector<float> dem((size_t)w * w, 1000.0f);
    uint32_t idx = 0u, ei = 0u, ej = 0u;
    for (uint32_t k = 0u, j = 0u; j < n; k++, j += 2u) {
        for (uint32_t c = 0u; c < n; c++) ei = (k & 1u) ? n - 1u - c : c, ej = j, dem[(size_t)(ej + 1u) * w + ei + 1u] = 0.25f * (float)idx++;
        if (j + 2u < n) dem[(size_t)(j + 2u) * w + ei + 1u] = 0.25f * (float)idx++;
    }
    for (uint32_t c = 0u; c < w; c++) dem[c] = dem[(size_t)(w - 1u) * w + c] = dem[(size_t)c * w] = dem[(size_t)c * w + w - 1u] = 2000.0f;
    dem[(size_t)(ej + 2u) * w + ei + 1u] = 0.25f * (float)(idx - 1u) + 1.0f;  // the gap: below the channel's end on the map, above it in height
    HostTables t = build_tables_host(dem.data(), w, w, 1.0f);  // (exaggeration 1: the table holds the DEM's bits)
    TerrainDev T{};
    t.attach(T);
    T.spacing_x = T.spacing_z = 10.0f;
    T.origin_x = T.origin_z = -0.5f * ((float)w - 1.0f) * 10.0f;
    const uint32_t whole[4] = {0u, 0u, w, w};
    const size_t m = (size_t)w * w;
    unsigned long long bad = 0ull;
    std::vector<float> W0(m), D0(m);
    std::vector<uint32_t> T0(m), acc0(m), basin0(m);
    std::vector<uint8_t> dir0(m);
    uint32_t fstats0[4] = {0u, 0u, 0u, 0u}, dstats0[3] = {0u, 0u, 0u};
    uint64_t segments0 = 0u;
    for (int run = 0; run < 4; run++) {
        const uint32_t edge = (run & 1) ? kFillTile : 8u, seed = (run & 2) ? 5u : 0u;
        std::vector<float> W(m), D(m);
        std::vector<uint32_t> Tf(m), acc(m), basin(m);
        std::vector<uint8_t> dir(m);
        uint32_t fstats[4], dstats[3];
        run_fill(T, edge, seed, whole, W.data(), D.data(), Tf.data(), fstats);
        run_drainage(T, edge, seed, whole, dir.data(), acc.data(), basin.data(), dstats);
        std::vector<float> seg(4u * m);
        const uint64_t segments = run_streams(T, edge, seed, whole, 2u, m, seg.data(), nullptr, nullptr, nullptr);
        unsigned long long sum = 0ull;
        for (size_t v = 0; v < m; v++) {
            const uint32_t i = (uint32_t)(v % w), j = (uint32_t)(v / w);
            bad += !(W[v] >= dem[v]) || D[v] != W[v] - dem[v] || Tf[v] == kFlatFar;
            if (dir[v] == kDrainSink) sum += acc[v], bad += !fill_outlet(w, w, i, j) || basin[v] != v;
        }
        bad += sum != m;
        if (run == 0) {
            W0 = W, D0 = D, T0 = Tf, acc0 = acc, basin0 = basin, dir0 = dir, segments0 = segments;
            for (int k = 0; k < 4; k++) fstats0[k] = fstats[k];
            for (int k = 0; k < 3; k++) dstats0[k] = dstats[k];
        }
        bad += W != W0 || D != D0 || Tf != T0 || acc != acc0 || basin != basin0 || dir != dir0 || segments != segments0;
        bad += fstats[0] != fstats0[0] || fstats[3] != fstats0[3] || dstats[0] != dstats0[0] || dstats[1] != dstats0[1] || dstats[2] != dstats0[2];
    }
    bad += fstats0[0] != 577u || fstats0[3] != 544u || dstats0[0] != 1u || dstats0[2] != 545u;
    printf("fill driver: %u filled, largest T %u, %u sinks, longest %u, %llu segments, disagreements: %llu\n", fstats0[0], fstats0[3], dstats0[0], dstats0[2],
           (unsigned long long)segments0, bad);
    return bad == 0ull ? 0 : 1;
}
#endif
