// tests/reterrain_host/reterrain_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_reterrain_host.py compiles it).
// The table passes of a re-terrain (f3d_retable.h: what k_retable_tiles / k_retable_top run per thread) on the host, over
// tables the product's own builder bodies made (leaf_build_at / level_build_at / band_build_at, as build_tables launches
// them), patched by a chain of blocks.  The bodies run one "thread" after the other in a shuffled order -- the tiles of a
// launch shuffled, the items between two barriers shuffled, the tile's LDS full of NaNs before its first item -- so nothing
// may depend on an order the device does not give.  After EVERY block:
//   (i)  the leaf table and every band level equal, byte for byte, the tables built from scratch for the edited DEM;
//   (ii) the same block is applied a second time to a copy whose records OUTSIDE the dirty range hold a poison pattern:
//        every one of them must still hold it afterwards (what a pass writes does not depend on what it reads).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../forge3d_amd/csrc/f3d_setup.h"
#include "../../forge3d_amd/csrc/f3d_retable.h"

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
    std::vector<uint32_t> order(uint32_t n) {
        std::vector<uint32_t> v(n);
        std::iota(v.begin(), v.end(), 0u);
        for (uint32_t i = n; i > 1u; i--) std::swap(v[i - 1u], v[next() % i]);
        return v;
    }
};

struct Tables {
    TableLayout L;
    std::vector<LeafRec> leaves;
    std::vector<NodeRec> bands;
};

// build_tables (f3d_host_mem.h) on the host: every record of every launch
Tables build(const float *dem, uint32_t w, uint32_t h, float exaggeration) {
    Tables t;
    t.L = table_layout(w, h);
    const TableLayout &L = t.L;
    t.leaves.assign(L.leaf_count, LeafRec{-7.0f, -7.0f, -7.0f, -7.0f});
    std::vector<NodeRec> nodes(L.node_count ? L.node_count : 1, NodeRec{-7.0f, -7.0f});
    t.bands.assign(L.band_count, NodeRec{-7.0f, -7.0f});
    const PyramidBuildParams B = leaf_build_params(L, dem, w, h, exaggeration, t.leaves.data());
    for (uint32_t y = 0; y < B.leaf_dim_y; y++)
        for (uint32_t x = 0; x < B.leaf_dim_x; x++) leaf_build_at(B, x, y);
    for (uint32_t l = 1; l < L.levels; l++) {
        const LevelBuildParams V = level_build_params(L, l, t.leaves.data(), nodes.data());
        for (uint32_t y = 0; y < V.dst_dim_y; y++)
            for (uint32_t x = 0; x < V.dst_dim_x; x++) level_build_at(V, x, y);
    }
    for (uint32_t l = 0; l < L.levels; l++) {
        const BandBuildParams V = band_build_params(L, l, t.leaves.data(), nodes.data(), t.bands.data());
        for (uint32_t z = 0; z < V.height; z++)
            for (uint32_t x = 0; x < V.width; x++) band_build_at(V, x, z);
    }
    return t;
}

// both launches of launch_retable, threads in a shuffled order
void apply(Tables &t, const float *block, uint32_t x0, uint32_t y0, uint32_t bw, uint32_t bh, float exaggeration, Rng &rng, RetableParams *out) {
    const RetableParams P = retable_params(t.L, block, x0, y0, bw, bh, exaggeration, t.leaves.data(), t.bands.data());
    if (out) *out = P;
    const uint32_t tile_levels = P.levels < kRetableTileLevels ? P.levels : kRetableTileLevels;
    for (uint32_t tile : rng.order(P.tiles_x * P.tiles_y)) {
        std::vector<NodeRec> lds(kRetableTileRecords, NodeRec{NAN, NAN});
        for (uint32_t i : rng.order(kRetableTile * kRetableTile)) retable_tile_level0(P, tile, lds.data(), i);
        for (uint32_t l = 1u; l < tile_levels; l++) {
            const uint32_t n = kRetableTile >> l;
            for (uint32_t i : rng.order(n * n)) retable_tile_level(P, tile, lds.data(), l, i);
        }
    }
    for (uint32_t l = kRetableTileLevels; l < P.levels; l++)
        for (uint32_t k : rng.order(retable_top_count(P, l))) retable_top_at(P, l, k);
}

constexpr uint32_t kPoison = 0x7FC5A5A5u;  // (a NaN: the reductions read it without trapping)

}  // namespace

// dem: w x h; n blocks: rects[4 i ..] = x0, y0, bw, bh, their samples back to back in `samples`; exaggerations[i]: 0 = keep
// (another value: the block is the whole DEM).  out[0] leaf records that differ from the scratch build, [1] band records,
// [2] poisoned records outside the dirty range that were written, [3] records compared, [4] dirty cells, [5] tile
// workgroups.  levels_out (optional): the band levels after the last block, level by level, level_h x level_w x (min, max),
// rows the band tables do not store as (+inf, -inf): the reference's chain.  dem (in / out): edited in place.
extern "C" int reterrain_chain(float *dem, uint32_t w, uint32_t h, float exaggeration, uint32_t n, const uint32_t *rects, const float *samples,
                               const float *exaggerations, uint64_t seed, uint64_t *out, float *levels_out) {
    if (w < 2u || h < 2u) return 1;
    Rng rng{seed};
    Tables t = build(dem, w, h, exaggeration);
    const TableLayout &L = t.L;
    for (int k = 0; k < 6; k++) out[k] = 0;
    for (uint32_t b = 0; b < n; b++) {
        const uint32_t x0 = rects[4u * b], y0 = rects[4u * b + 1u], bw = rects[4u * b + 2u], bh = rects[4u * b + 3u];
        if (bw == 0u || bh == 0u || x0 >= w || y0 >= h || bw > w - x0 || bh > h - y0) return 2;
        if (exaggerations[b] != 0.0f) {
            if (!(x0 == 0u && y0 == 0u && bw == w && bh == h)) return 3;
            exaggeration = exaggerations[b];
        }
        for (uint32_t y = 0; y < bh; y++)
            for (uint32_t x = 0; x < bw; x++) dem[(size_t)(y0 + y) * w + x0 + x] = samples[(size_t)y * bw + x];
        // (ii) first, on a poisoned copy of the tables as they are
        Tables p = t;
        RetableParams P{};
        {
            const RetableParams Q = retable_params(L, samples, x0, y0, bw, bh, exaggeration, p.leaves.data(), p.bands.data());
            const LeafRec bad_leaf{f_from_bits(kPoison), f_from_bits(kPoison), f_from_bits(kPoison), f_from_bits(kPoison)};
            const NodeRec bad_node{f_from_bits(kPoison), f_from_bits(kPoison)};
            std::vector<uint8_t> keep(L.leaf_count, 0);
            for (uint32_t y = Q.lo_y; y <= Q.hi_y; y++)
                for (uint32_t x = Q.lo_x; x <= Q.hi_x; x++) keep[tiled_index(x, y, L.tiles_x[0])] = 1;
            for (size_t i = 0; i < L.leaf_count; i++)
                if (!keep[i]) p.leaves[i] = bad_leaf;
            for (uint32_t l = 0; l < L.levels; l++)
                for (uint32_t y = 0; y < L.band_rows[l]; y++)
                    for (uint32_t x = 0; x < L.level_w[l]; x++)
                        if (!retable_dirty(Q, l, x, y)) p.bands[L.band_offset[l] + ((size_t)y << L.band_shift[l]) + x] = bad_node;
            apply(p, samples, x0, y0, bw, bh, exaggeration, rng, &P);
            for (size_t i = 0; i < L.leaf_count; i++)
                if (!keep[i] && memcmp(&p.leaves[i], &bad_leaf, sizeof bad_leaf) != 0) out[2]++;
            for (uint32_t l = 0; l < L.levels; l++)
                for (uint32_t y = 0; y < L.band_rows[l]; y++)
                    for (uint32_t x = 0; x < L.level_w[l]; x++)
                        if (!retable_dirty(Q, l, x, y) &&
                            memcmp(&p.bands[L.band_offset[l] + ((size_t)y << L.band_shift[l]) + x], &bad_node, sizeof bad_node) != 0)
                            out[2]++;
        }
        // (i) the real tables against a build from scratch
        apply(t, samples, x0, y0, bw, bh, exaggeration, rng, nullptr);
        const Tables want = build(dem, w, h, exaggeration);
        for (size_t i = 0; i < L.leaf_count; i++)
            if (memcmp(&t.leaves[i], &want.leaves[i], sizeof(LeafRec)) != 0) out[0]++;
        for (size_t i = 0; i < L.band_count; i++)
            if (memcmp(&t.bands[i], &want.bands[i], sizeof(NodeRec)) != 0) out[1]++;
        out[3] += L.leaf_count + L.band_count;
        out[4] += (uint64_t)(P.hi_x - P.lo_x + 1u) * (P.hi_y - P.lo_y + 1u);
        out[5] += (uint64_t)P.tiles_x * P.tiles_y;
        samples += (size_t)bw * bh;
    }
    if (levels_out) {
        for (uint32_t l = 0; l < L.levels; l++)
            for (uint32_t y = 0; y < L.level_h[l]; y++)
                for (uint32_t x = 0; x < L.level_w[l]; x++) {
                    NodeRec r{__builtin_inff(), -__builtin_inff()};
                    if (y < L.band_rows[l]) r = t.bands[L.band_offset[l] + ((size_t)y << L.band_shift[l]) + x];
                    *levels_out++ = r.mn;
                    *levels_out++ = r.mx;
                }
    }
    return 0;
}

// The comparison can fail: the same chain with the level passes left out (leaves and level 0 only) -- out[1] must see it.
extern "C" int reterrain_stale(float *dem, uint32_t w, uint32_t h, float exaggeration, const uint32_t *rect, const float *samples, uint64_t *out) {
    Tables t = build(dem, w, h, exaggeration);
    const uint32_t x0 = rect[0], y0 = rect[1], bw = rect[2], bh = rect[3];
    for (uint32_t y = 0; y < bh; y++)
        for (uint32_t x = 0; x < bw; x++) dem[(size_t)(y0 + y) * w + x0 + x] = samples[(size_t)y * bw + x];
    const RetableParams P = retable_params(t.L, samples, x0, y0, bw, bh, exaggeration, t.leaves.data(), t.bands.data());
    for (uint32_t y = P.lo_y; y <= P.hi_y; y++)
        for (uint32_t x = P.lo_x; x <= P.hi_x; x++) retable_leaf_at(P, x, y);
    const Tables want = build(dem, w, h, exaggeration);
    out[0] = out[1] = 0;
    for (size_t i = 0; i < t.L.leaf_count; i++)
        if (memcmp(&t.leaves[i], &want.leaves[i], sizeof(LeafRec)) != 0) out[0]++;
    for (size_t i = 0; i < t.L.band_count; i++)
        if (memcmp(&t.bands[i], &want.bands[i], sizeof(NodeRec)) != 0) out[1]++;
    return 0;
}
