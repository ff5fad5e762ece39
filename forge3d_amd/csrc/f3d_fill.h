// forge3d_amd/csrc/f3d_fill.h -- drainage through depressions (f3d_session_fill, and F3D_DRAINAGE_FILL on the drainage entries):
// the filled surface, the distance across its flats and the D8 rule on both -- what one lane of k_fill_init, k_flat_init,
// k_fill_direction, k_fill_stats and k_fill_write does for its sample, and what one thread of a workgroup of k_fill_relax /
// k_flat_relax does for its tile.  Host and device: tests/fill_host runs the same bodies on the CPU, the threads of a tile one
// after the other, the tiles of a round in index order or in a permuted one, and the device returns those bits.
//
// THE CONTRACT.  All arithmetic is f32, one rounding per operation, as in f3d_drainage.h.
//
// Samples, the neighbour order (E, SE, S, SW, W, NW, N, NE = 0 .. 7), run_k, diag and lattice_height are f3d_drainage.h's.
// Heights are finite: a session refuses others at upload, so there is no NaN rule.  z is lattice_height + 0.0f: a height of
// -0 is taken as +0, so that values that compare equal have equal bits and a selection among them cannot show in the result.
//
// Outlets.  A sample on the grid's first or last row or column is an OUTLET.
//
// Filled surface W (f32).  W = z on outlets; elsewhere
//      W(c) = max(z(c), min over the existing neighbours n of W(n)),
// taken as the GREATEST solution: the least, over all 8-connected paths from c to an outlet, of the highest sample on the path
// -- what priority-flood computes.  It is computed by relaxation from W0 = z on outlets and +inf elsewhere.  The operator is
// monotone and only SELECTS among input values (min and max never round), so every W ever stored is one of the DEM's heights or
// +inf, every stored value is an upper bound of the solution, and any order of updates, with reads that see old or new values,
// ends in the same bits.  THE CONTRACT IS THE FIXED POINT, NOT THE SCHEDULE.  depth = W - z (one f32 subtraction) is the water
// depth of the lakes.
//
// Flat distance T (uint32).  T = 0 on outlets and on samples with a neighbour of strictly smaller W (f32 compare); elsewhere
//      T(c) = 1 + min T(n) over the neighbours with W(n) == W(c):
// the BFS distance, within a plateau of the filled surface, to where the plateau drains.  The same kind of monotone relaxation,
// from 0 and 0xFFFFFFFF (1 + 0xFFFFFFFF stays 0xFFFFFFFF).
// Every sample gets a finite T: for an undrained c the fixed-point identity gives min_n W(n) == W(c) (min_n W(n) >= W(c) since
// no neighbour is lower, and W(c) > min_n W(n) would need W(c) = z(c) > every path's bound, i.e. W(c) > W(c)).  Walk a minimax
// path from c: its prefix up to the first sample of smaller W, or up to its outlet, lies in c's plateau and ends on a sample
// with T = 0.
//
// Direction on the filled surface.  First drain_direction's rule on W: the largest slope_k = (W(c) - W(n_k)) / run_k > 0, ties
// to the lowest k.  If there is none and c is an outlet: a sink, code 8.  If there is none and c is no outlet: the lowest k
// with W(n_k) < W(c), or with W(n_k) == W(c) and T(n_k) < T(c).  The last rule always finds a neighbour -- a sample with T = 0
// that is no outlet has a strictly lower neighbour, one with T > 0 has a neighbour of its plateau with T - 1 -- and does not
// depend on a quotient that could underflow to 0.
// THE RECEIVERS FORM A FOREST WHOSE ROOTS ARE EXACTLY THE OUTLETS WITHOUT A POSITIVE SLOPE.  A positive slope goes to a
// strictly smaller W (f3d_drainage.h's argument); the last rule goes to a smaller W or to an equal W and a smaller T.  Every
// step lowers the key (W, T) lexicographically, so no sample comes twice and every path ends; it can only end on a sample the
// rules leave without a receiver, and those are outlets.  No interior sample is a sink.
//
// Accumulation, basin, depth, longest, rounds and the streams are f3d_drainage.h's, over these receivers: k_drain_jump,
// k_drain_add, k_drain_write and k_stream_* run as they are.
//
// THE RELAXATION BY TILES.  The grid is cut into square tiles of E x E samples (kFillTile on the device).  A workgroup of 4 E
// threads stages its tile's two planes -- the fixed one (z, or W) and the relaxed one (W, or T) -- with a one-sample halo into
// LDS, then sweeps: thread t owns line t % E in direction t / E (rows eastward, rows westward, columns southward, columns
// northward) and walks it sample by sample, so a value crosses the tile within one sweep; the four directions run side by
// side.  A sample is only ever lowered (`candidate < old`).  Sweeps repeat until one changes nothing -- then every sample of
// the tile satisfies its equation against the staged halo.  The threads of a sweep read each other's words old or new: both
// are upper bounds of the fixed point, and a sweep that lowered anything is followed by another.  Across tiles likewise: a
// halo read sees the neighbour tile's value of the round before or of this round, both upper bounds; a tile whose edge sample
// changed marks the up to eight tiles that stage it dirty for the next round, so whoever read the old value runs again.  A
// round that marks nothing has every tile at rest against final halos: the fixed point.  Termination: every mark follows a
// lowered value drawn from a finite set.  There is no round cap.
// Dirty flags are words, two planes: round r reads and clears plane r & 1 and marks plane (r + 1) & 1; the number of tiles
// newly marked goes into the slotted counter set (r + 1) & 1 (kDrainSlots words, f3d_drainage.h's idiom), which the host sums
// after the round; tile 0 clears set r & 1, that the host has read, for round r + 1.
// An LDS row is (E + 2) | 1 words: odd, so that the 32 lanes of a row sweep (one row each, the same column) fall on 32 banks,
// as the 32 lanes of a column sweep (one column each, the same row) do anyway.
#pragma once

#include "f3d_drainage.h"

namespace f3d {

constexpr uint32_t kFillTile = 64u;              // the device's tile edge (profiles/README.md)
constexpr uint32_t kFlatFar = 0xFFFFFFFFu;       // T before it is known
// counters (uint32 words, zeroed before a call), kDrainSlots words each: two sets of "tiles marked for the next round", the
// samples with W > z, the largest T
constexpr uint32_t kFillMarks = 0u, kFillFilled = 2u * kDrainSlots, kFillLargest = 3u * kDrainSlots, kFillCounters = 4u * kDrainSlots;

struct FillParams {
    TerrainDev terrain;
    uint32_t w, h;             // samples a row, rows
    uint32_t tile;             // E
    uint32_t round;            // r of the relax kernels
    float *z, *W;              // w * h words each
    uint32_t *T;               // w * h words
    uint32_t *dirty[2];        // fill_tiles() words each
    uint32_t *counters;        // kFillCounters words
    // the region written back (k_fill_write)
    uint32_t row0, col0, rows, cols;
    float *out_filled, *out_depth;   // rows * cols, or null
    uint32_t *out_flat;
};

F3D_HD float fill_inf() { return __builtin_huge_valf(); }
F3D_HD float fill_nan() { return __builtin_nanf(""); }
F3D_HD bool fill_outlet(uint32_t w, uint32_t h, uint32_t i, uint32_t j) { return i == 0u || j == 0u || i + 1u == w || j + 1u == h; }
F3D_HD uint32_t fill_tiles_x(uint32_t w, uint32_t e) { return (w + e - 1u) / e; }
F3D_HD uint32_t fill_tiles(uint32_t w, uint32_t h, uint32_t e) { return fill_tiles_x(w, e) * ((h + e - 1u) / e); }

// k_fill_init's lane: z materialised (4 bytes a sample, read by every round's staging instead of the leaf table's 16-byte
// records), W0; the first fill_tiles() lanes mark their tile dirty in plane 0 and clear plane 1.
F3D_HD void fill_lane_init(const FillParams &P, uint32_t v) {
    const uint32_t j = v / P.w, i = v - j * P.w;
    const float z = lattice_height(P.terrain, i, j) + 0.0f;  // (-0 becomes +0)
    P.z[v] = z;
    P.W[v] = fill_outlet(P.w, P.h, i, j) ? z : fill_inf();
    if (v < fill_tiles(P.w, P.h, P.tile)) P.dirty[0][v] = 1u, P.dirty[1][v] = 0u;
}

// k_flat_init's lane: T0, and whether the sample is undrained (its tile then starts dirty in plane 0).  The fill pass leaves
// both dirty planes and both counter sets clear.
F3D_HD bool flat_lane_init(const FillParams &P, uint32_t v) {
    const uint32_t j = v / P.w, i = v - j * P.w;
    const float here = P.W[v];
    bool drained = fill_outlet(P.w, P.h, i, j);
    for (uint32_t k = 0u; k < 8u && !drained; k++) {
        const uint32_t ni = i + (uint32_t)drain_di(k), nj = j + (uint32_t)drain_dj(k);
        if (ni < P.w && nj < P.h && P.W[nj * P.w + ni] < here) drained = true;
    }
    P.T[v] = drained ? 0u : kFlatFar;
    return !drained;
}
F3D_HD uint32_t fill_tile_of(const FillParams &P, uint32_t v) {
    const uint32_t j = v / P.w, i = v - j * P.w;
    return (j / P.tile) * fill_tiles_x(P.w, P.tile) + i / P.tile;
}

// The two relaxations' rules over a staged tile: a = the fixed plane, b = the relaxed one, at = the sample's word, S = the row
// stride.  outside_*: what a slot beyond the grid holds -- values that neither lower a neighbour nor are ever lowered.
struct FillRule {
    typedef float A;
    typedef float B;
    static F3D_HD A outside_a() { return fill_inf(); }
    static F3D_HD B outside_b() { return fill_inf(); }
    static F3D_HD const A *plane_a(const FillParams &P) { return P.z; }
    static F3D_HD B *plane_b(const FillParams &P) { return P.W; }
    static F3D_HD B candidate(const A *a, const B *b, uint32_t at, uint32_t S) {
        float low = b[at + 1u];
        for (uint32_t k = 1u; k < 8u; k++) {
            const float n = b[(int32_t)at + drain_dj(k) * (int32_t)S + drain_di(k)];
            low = n < low ? n : low;
        }
        const float z = a[at];
        return z > low ? z : low;
    }
};
struct FlatRule {
    typedef float A;
    typedef uint32_t B;
    static F3D_HD A outside_a() { return fill_nan(); }   // (equal to nothing)
    static F3D_HD B outside_b() { return kFlatFar; }
    static F3D_HD const A *plane_a(const FillParams &P) { return P.W; }
    static F3D_HD B *plane_b(const FillParams &P) { return P.T; }
    static F3D_HD B candidate(const A *a, const B *b, uint32_t at, uint32_t S) {
        const float here = a[at];
        uint32_t low = kFlatFar;
        for (uint32_t k = 0u; k < 8u; k++) {
            const uint32_t n = (uint32_t)((int32_t)at + drain_dj(k) * (int32_t)S + drain_di(k));
            if (a[n] == here && b[n] < low) low = b[n];
        }
        return low == kFlatFar ? kFlatFar : low + 1u;
    }
};

// One tile of E x E samples in the hands of 4 E threads.
template <uint32_t E, class Rule>
struct FillTileBody {
    typedef typename Rule::A A;
    typedef typename Rule::B B;
    static constexpr uint32_t kThreads = 4u * E, kSide = E + 2u, kStride = (E + 2u) | 1u, kWords = kSide * kStride;

    // thread t's share of the staging: the tile and its halo out of the two planes
    static F3D_HD void load(const FillParams &P, uint32_t tile, uint32_t t, A *a, B *b) {
        const uint32_t tiles_x = fill_tiles_x(P.w, E), i0 = (tile % tiles_x) * E, j0 = (tile / tiles_x) * E;
        const A *pa = Rule::plane_a(P);
        const B *pb = Rule::plane_b(P);
        for (uint32_t n = t; n < kSide * kSide; n += kThreads) {
            const uint32_t ly = n / kSide, lx = n - ly * kSide;
            const uint32_t i = i0 + lx - 1u, j = j0 + ly - 1u;  // (below 0 wraps above w, h)
            const bool have = i < P.w && j < P.h;
            a[ly * kStride + lx] = have ? pa[(size_t)j * P.w + i] : Rule::outside_a();
            b[ly * kStride + lx] = have ? pb[(size_t)j * P.w + i] : Rule::outside_b();
        }
    }

    // thread t's line of one sweep; returns whether it lowered a sample
    static F3D_HD bool sweep(uint32_t t, const A *a, B *b) {
        const uint32_t dir = t / E, line = t - dir * E;
        bool changed = false;
        for (uint32_t step = 0u; step < E; step++) {
            const uint32_t pos = (dir & 1u) ? E - 1u - step : step;
            const uint32_t lx = dir < 2u ? pos : line, ly = dir < 2u ? line : pos;
            const uint32_t at = (ly + 1u) * kStride + lx + 1u;
            const B old = b[at], cand = Rule::candidate(a, b, at, kStride);
            if (cand < old) b[at] = cand, changed = true;
        }
        return changed;
    }

    // thread t's share of the write-back: its samples that changed go to the relaxed plane; returns the neighbour tiles
    // (bit k: the one in direction k) that stage one of them in their halo
    static F3D_HD uint32_t store(const FillParams &P, uint32_t tile, uint32_t t, const B *b) {
        const uint32_t tiles_x = fill_tiles_x(P.w, E), i0 = (tile % tiles_x) * E, j0 = (tile / tiles_x) * E;
        B *pb = Rule::plane_b(P);
        uint32_t touched = 0u;
        for (uint32_t n = t; n < E * E; n += kThreads) {
            const uint32_t ly = n / E, lx = n - ly * E, i = i0 + lx, j = j0 + ly;
            if (i >= P.w || j >= P.h) continue;
            const B now = b[(ly + 1u) * kStride + lx + 1u];
            if (now == pb[(size_t)j * P.w + i]) continue;
            pb[(size_t)j * P.w + i] = now;
            for (uint32_t k = 0u; k < 8u; k++) {
                const int32_t di = drain_di(k), dj = drain_dj(k);
                const bool x = di == 0 || (di > 0 ? lx == E - 1u : lx == 0u), y = dj == 0 || (dj > 0 ? ly == E - 1u : ly == 0u);
                if (x && y) touched |= 1u << k;
            }
        }
        return touched;
    }

    // the tile in direction k of `tile`, or false
    static F3D_HD bool neighbour(const FillParams &P, uint32_t tile, uint32_t k, uint32_t &other) {
        const uint32_t tiles_x = fill_tiles_x(P.w, E), tiles_y = (P.h + E - 1u) / E;
        const uint32_t tx = tile % tiles_x + (uint32_t)drain_di(k), ty = tile / tiles_x + (uint32_t)drain_dj(k);
        other = ty * tiles_x + tx;
        return tx < tiles_x && ty < tiles_y;
    }
};

// The D8 code of sample (i, j) on the filled surface: 0 .. 7, or kDrainSink on an outlet without a positive slope.
F3D_HD uint32_t fill_direction(const TerrainDev &T, uint32_t w, uint32_t h, float diag, const float *W, const uint32_t *flat, uint32_t i, uint32_t j) {
    const uint32_t v = j * w + i;
    const float here = W[v];
    float best = 0.0f;
    uint32_t code = kDrainSink;
    for (uint32_t k = 0u; k < 8u; k++) {
        const uint32_t ni = i + (uint32_t)drain_di(k), nj = j + (uint32_t)drain_dj(k);
        if (ni >= w || nj >= h) continue;
        const float run = (k & 1u) ? diag : ((k & 2u) ? T.spacing_z : T.spacing_x);
        const float slope = (here - W[nj * w + ni]) / run;
        if (slope > best) best = slope, code = k;
    }
    if (code != kDrainSink || fill_outlet(w, h, i, j)) return code;
    const uint32_t far = flat[v];
    for (uint32_t k = 0u; k < 8u; k++) {
        const uint32_t ni = i + (uint32_t)drain_di(k), nj = j + (uint32_t)drain_dj(k);
        if (ni >= w || nj >= h) continue;
        const float there = W[nj * w + ni];
        if (there < here || (there == here && flat[nj * w + ni] < far)) return k;
    }
    return kDrainSink;  // (not reached: the contract's last rule always finds a neighbour)
}

// k_fill_direction's lane: drain_lane_direction with the rule above.  Returns whether the sample is a sink.
F3D_HD bool fill_lane_direction(const DrainParams &P, uint32_t i, uint32_t j) {
    const uint32_t code = fill_direction(P.terrain, P.w, P.h, P.diag, P.fill_W, P.fill_T, i, j), v = j * P.w + i;
    P.code[v] = (uint8_t)code;
    P.q[v] = drain_receiver(P.w, i, j, code) | (code == kDrainSink ? 0u : kDrainLive);
    P.s[v] = 1u;
    P.depth[v] = 0u;
    return code == kDrainSink;
}

// k_fill_stats' lane: is the sample filled; its T
F3D_HD bool fill_lane_stats(const FillParams &P, uint32_t v, uint32_t &flat) {
    flat = P.T[v];
    return P.W[v] > P.z[v];
}

// k_fill_write's lane: sample n of the region
F3D_HD void fill_lane_write(const FillParams &P, uint32_t n) {
    const uint32_t r = n / P.cols, v = (P.row0 + r) * P.w + P.col0 + (n - r * P.cols);
    if (P.out_filled) P.out_filled[n] = P.W[v];
    if (P.out_depth) P.out_depth[n] = P.W[v] - P.z[v];
    if (P.out_flat) P.out_flat[n] = P.T[v];
}

}  // namespace f3d
