// forge3d_amd/csrc/f3d_drainage.h -- drainage of a live session's terrain (f3d_session_drainage, f3d_session_streams,
// f3d_session_paint_streams): what one lane of k_drain_direction, k_drain_jump, k_drain_add, k_drain_write, k_stream_count and
// k_stream_emit does for its sample.  Host and device: tests/drainage_host runs the same bodies on the CPU over whole 64-lane
// waves, the rounds as Jacobi sweeps, and the device returns those bits, in that order.
//
// THE CONTRACT.  All arithmetic is f32, one rounding per written operation (the library and the host harness are compiled with
// -ffp-contract=off; the only fused multiply-add is plane_at's own, the lattice's); division is the correctly rounded form.
//
// Samples.  The DEM's samples are (i, j), i < w = cell_w + 1 (+i east), j < h = cell_h + 1 (+j south); the linear index is
// j * w + i.  A sample's height is lattice_height(T, i, j): the leaf table's corner with the exaggeration applied, the y that
// ground() returns.
//
// Direction (D8).  The neighbours are taken in the fixed order E, SE, S, SW, W, NW, N, NE = codes 0 .. 7; a neighbour outside
// the grid does not exist.  run_k is spacing_x for E and W, spacing_z for N and S and, for the four diagonals,
//      diag = sqrt(spacing_x * spacing_x + spacing_z * spacing_z)
// formed ONCE per call on the host in f32 -- two products, one sum, one correctly rounded sqrt -- and handed to every lane.
//      slope_k = (hgt(i, j) - hgt(neighbour_k)) / run_k
// The direction is the k with the largest slope_k > 0; of equal slopes the lowest k wins (the lane keeps a candidate only when
// it is strictly greater than the best so far).  A sample with no slope_k > 0 is a SINK, code 8: pits, flats and the border's
// outlets alike.  A NaN height compares false everywhere: the sample is a sink and nobody drains into it.
//
// THE RECEIVERS FORM A FOREST, rooted at the sinks.  spacing_x, spacing_z (checked > 0 at the session's creation) and diag are
// positive, so slope_k > 0 implies hgt(i, j) - hgt(neighbour) > 0 as rounded, and a rounded difference is positive only when
// hgt(i, j) > hgt(neighbour) as f32 values (the subtraction is monotone and exact at zero).  Every step of a path therefore
// goes to a strictly lower f32 height; heights along a path strictly decrease, no sample can come twice, every path ends in
// a sink after fewer than w * h steps.  No cycle check is needed and none is made.
//
// Accumulation, uint32: the number of samples whose path passes through the sample, itself included (1 where nothing drains
// in).  The sinks' accumulations sum to w * h.  Basin, uint32: the linear index of the sink the sample's path ends in; a sink
// labels itself.  THE WHOLE DEM IS ALWAYS ROUTED: what drains through a region depends on what lies outside it.  `region` is a
// region of SAMPLES (row0, col0, rows, cols), as the visibility rasters'; it selects what is written back, sample n = r * cols + c.
//
// ACCUMULATION BY PATH DOUBLING.  Per sample v and round k = 0, 1, ...:
//      q_k[v]     the ancestor of v at distance min(2^k, depth(v))           (q_0: the receiver; a sink: itself)
//      live_k[v]  depth(v) >= 2^k                                             (live_0: not a sink)
//      s_k[v]     the samples of v's subtree at distance < 2^k from v         (s_0 = 1)
// One round is a Jacobi step from (q_k | live_k, s_k) into a second pair of planes:
//      s_k+1[v] = s_k[v] + sum of s_k[u] over the u with live_k[u] and q_k[u] = v
//          (a live u's q_k[u] lies exactly 2^k above it; the samples at distance [2^k, 2^(k+1)) below v are those at distance
//          < 2^k below such a u) -- k_drain_jump copies s_k[v], then in k_drain_add a live lane does ONE integer atomicAdd of
//          s_k[u] into s_k+1[q_k[u]].  Integer sums do not depend on the order of arrival: the result is the same bits
//          whatever the device schedules, which a float weight would not give (and is why there is none);
//      q_k+1[v] = q_k[q_k[v]]        live_k+1[v] = live_k[v] && live_k[q_k[v]]
// When no sample is live, s is the accumulation and q the basin.  Round k has a live sample iff the longest path has L >= 2^k
// steps: floor(log2 L) + 1 rounds for L > 0, none on a flat.  The host reads "live samples of the next round" back after every
// round and stops at 0; `rounds` is the number of rounds that had a live sample.
// depth(v) itself falls out of the same sweep: a sample that is live in round k while its q_k[v] is not has
// depth(v) = 2^k + depth(q_k[v]), and depth(q_k[v]) < 2^k was written in an earlier round (a sink's 0 by k_drain_direction).
// `longest` = L is the maximum.
// THE LIVE BIT IS BIT 31 OF THE POINTER WORD, which leaves 31 bits for an index: w * h <= 2^31 = kDrainMaxSamples, and a larger
// DEM is refused (so is, with it, every w * h >= 2^32 that uint32 counts could not hold).
//
// Streams.  A sample with accumulation >= threshold (threshold >= 1) that is not a sink emits ONE segment, from its own lattice
// point to its receiver's,
//      (plane_at(origin_x, i, spacing_x), plane_at(origin_z, j, spacing_z))  ->  the same of (i + di, j + dj)
// with the sample's accumulation.  A sample belongs to a region's output iff it lies in the region; its receiver may lie
// outside.  The order is row-major over the region's samples and depends on nothing else.  Records: float[4] = (ax, az, bx, bz)
// and a parallel uint32 accumulation; or a PaintPrim exactly as f3d_contour.h builds one (contour_prim: v = (a, b, b), the
// call's colour, feature 0).  Two passes as the contours': a wave owns 64 consecutive samples of the region, counts, the
// contours' exclusive scan over the waves' totals, then every lane writes at its wave's offset plus its wave-exclusive prefix.
#pragma once

#include "f3d_contour.h"
#include "f3d_walk.h"

namespace f3d {

constexpr uint64_t kDrainMaxSamples = 1ull << 31;
constexpr uint32_t kDrainSink = 8u, kDrainLive = 0x80000000u, kDrainIndex = 0x7FFFFFFFu;
// counters (uint32 words, zeroed before a call), each kind spread over kDrainSlots words -- a wave adds into slot (wave & 255),
// the host sums or maximises the slots -- because 65 536 waves' atomics on ONE word queue behind each other (measured: 0.7 ms a
// round on the 2048^2 proxy): [kDrainSinks + slot] sinks, [kDrainLongest + slot] longest, [kDrainLiveAt + k * kDrainSlots + slot]
// live samples of round k
constexpr uint32_t kDrainSlots = 256u, kDrainMaxRounds = 32u;
constexpr uint32_t kDrainSinks = 0u, kDrainLongest = kDrainSlots, kDrainLiveAt = 2u * kDrainSlots, kDrainCounters = (3u + kDrainMaxRounds) * kDrainSlots;

struct DrainParams {
    TerrainDev terrain;
    uint32_t w, h;            // samples a row, rows
    float diag;               // drain_diag()
    uint32_t round;           // k of k_drain_jump / k_drain_add
    uint8_t *code;            // w * h bytes
    uint32_t *q, *s;          // round k's planes: pointer | live, subtree count
    uint32_t *q_next, *s_next;  // round k + 1's
    uint32_t *depth;          // w * h words, final once a sample is not live
    uint32_t *counters;       // kDrainCounters words
    // the region written back (k_drain_write) or emitted (k_stream_*)
    uint32_t row0, col0, rows, cols;
    uint8_t *out_direction;   // rows * cols, or null
    uint32_t *out_accumulation, *out_basin;
    uint32_t threshold;
    uint64_t *totals;          // waves + 1 words: segments a wave, then 0
    const uint64_t *offsets;   // their exclusive scan
    uint64_t capacity;
    float *segments;           // capacity x 4, or null
    uint32_t *stream_accumulation;  // capacity, or null
    PaintPrim *prims;          // capacity records, or null (then segments / stream_accumulation)
    float rgba[4];
    // the filled form (f3d_fill.h: k_fill_direction reads them); null: unfilled
    const float *fill_W;       // w * h words: the filled surface
    const uint32_t *fill_T;    // w * h words: the distance across its flats
};

// (host, once per call)
inline float drain_diag(float spacing_x, float spacing_z) {
    const float xx = spacing_x * spacing_x, zz = spacing_z * spacing_z;
    const float sum = xx + zz;
    return std::sqrt(sum);
}

F3D_HD int32_t drain_di(uint32_t k) { return (int32_t)((0x21000122u >> (4u * k)) & 15u) - 1; }  // 1, 1, 0, -1, -1, -1, 0, 1
F3D_HD int32_t drain_dj(uint32_t k) { return (int32_t)((0x00012221u >> (4u * k)) & 15u) - 1; }  // 0, 1, 1, 1, 0, -1, -1, -1

// The D8 code of sample (i, j): 0 .. 7, or kDrainSink.
F3D_HD uint32_t drain_direction(const TerrainDev &T, uint32_t w, uint32_t h, float diag, uint32_t i, uint32_t j) {
    const float here = lattice_height(T, i, j);
    float best = 0.0f;
    uint32_t code = kDrainSink;
    for (uint32_t k = 0u; k < 8u; k++) {
        const uint32_t ni = i + (uint32_t)drain_di(k), nj = j + (uint32_t)drain_dj(k);  // (below 0 wraps above w, h)
        if (ni >= w || nj >= h) continue;
        const float run = (k & 1u) ? diag : ((k & 2u) ? T.spacing_z : T.spacing_x);
        const float slope = (here - lattice_height(T, ni, nj)) / run;
        if (slope > best) best = slope, code = k;
    }
    return code;
}

F3D_HD uint32_t drain_receiver(uint32_t w, uint32_t i, uint32_t j, uint32_t code) {
    return code == kDrainSink ? j * w + i : (j + (uint32_t)drain_dj(code)) * w + (i + (uint32_t)drain_di(code));
}

// lane of the wave that owns tile `tile` of 8 x 8 samples (aligned to the leaf table's 8 x 8 tiles of cells: sample (i, j) is
// corner 0 of cell (i, j), so a wave's nine-point stencils read its own tile's records and a fringe of its neighbours')
F3D_HD bool drain_tile_sample(uint32_t w, uint32_t h, uint32_t tile, uint32_t lane, uint32_t &i, uint32_t &j) {
    const uint32_t tiles_x = (w + 7u) >> 3;
    i = (tile % tiles_x) * 8u + (lane & 7u);
    j = (tile / tiles_x) * 8u + (lane >> 3);
    return i < w && j < h;
}
F3D_HD uint32_t drain_tiles(uint32_t w, uint32_t h) { return ((w + 7u) >> 3) * ((h + 7u) >> 3); }

// k_drain_direction's lane: the code, round 0's planes, depth 0.  Returns whether the sample is a sink.
F3D_HD bool drain_lane_direction(const DrainParams &P, uint32_t i, uint32_t j) {
    const uint32_t code = drain_direction(P.terrain, P.w, P.h, P.diag, i, j), v = j * P.w + i;
    P.code[v] = (uint8_t)code;
    P.q[v] = drain_receiver(P.w, i, j, code) | (code == kDrainSink ? 0u : kDrainLive);
    P.s[v] = 1u;
    P.depth[v] = 0u;
    return code == kDrainSink;
}

// k_drain_jump's lane: round k + 1's pointer word and the copy of s; depth where it becomes known (`depth`, else 0).
// Returns whether v is live in round k + 1.
F3D_HD bool drain_lane_jump(const DrainParams &P, uint32_t v, uint32_t &depth) {
    const uint32_t qv = P.q[v], up = P.q[qv & kDrainIndex];
    const bool live = (qv & kDrainLive) != 0u, next = live && (up & kDrainLive) != 0u;
    P.q_next[v] = (up & kDrainIndex) | (next ? kDrainLive : 0u);
    P.s_next[v] = P.s[v];
    depth = 0u;
    if (live && !next) {
        depth = (1u << P.round) + P.depth[qv & kDrainIndex];
        P.depth[v] = depth;
    }
    return next;
}

// k_drain_add's lane: false -- nothing to add; else s_k[v] goes into s_k+1[target].
F3D_HD bool drain_lane_add(const DrainParams &P, uint32_t v, uint32_t &target, uint32_t &amount) {
    const uint32_t qv = P.q[v];
    if ((qv & kDrainLive) == 0u) return false;
    target = qv & kDrainIndex;
    amount = P.s[v];
    return true;
}

// sample n of the region -> (i, j); the planes read are the final ones (P.q, P.s)
F3D_HD void drain_region_sample(const DrainParams &P, uint32_t n, uint32_t &i, uint32_t &j) {
    const uint32_t r = n / P.cols;
    j = P.row0 + r;
    i = P.col0 + (n - r * P.cols);
}

// k_drain_write's lane
F3D_HD void drain_lane_write(const DrainParams &P, uint32_t n) {
    uint32_t i, j;
    drain_region_sample(P, n, i, j);
    const uint32_t v = j * P.w + i;
    if (P.out_direction) P.out_direction[n] = P.code[v];
    if (P.out_accumulation) P.out_accumulation[n] = P.s[v];
    if (P.out_basin) P.out_basin[n] = P.q[v] & kDrainIndex;
}

// k_stream_count's and k_stream_emit's lane: does sample n of the region emit?
F3D_HD bool stream_lane(const DrainParams &P, uint32_t n, uint32_t &i, uint32_t &j, uint32_t &code, uint32_t &accumulation) {
    if (n >= P.rows * P.cols) return false;
    drain_region_sample(P, n, i, j);
    const uint32_t v = j * P.w + i;
    code = P.code[v];
    accumulation = P.s[v];
    return code != kDrainSink && accumulation >= P.threshold;
}
F3D_HD uint32_t stream_waves(uint32_t rows, uint32_t cols) { return (rows * cols + 63u) >> 6; }

F3D_HD void stream_segment(const TerrainDev &T, uint32_t i, uint32_t j, uint32_t code, float &ax, float &az, float &bx, float &bz) {
    ax = plane_at(T.origin_x, i, T.spacing_x);
    az = plane_at(T.origin_z, j, T.spacing_z);
    bx = plane_at(T.origin_x, i + (uint32_t)drain_di(code), T.spacing_x);
    bz = plane_at(T.origin_z, j + (uint32_t)drain_dj(code), T.spacing_z);
}

}  // namespace f3d
