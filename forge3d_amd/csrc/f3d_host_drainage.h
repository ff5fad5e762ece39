// f3d_host_drainage.h -- part of f3d_host.hip (included there once, after the contours): drainage of a live session's terrain
// (the lanes' bodies are f3d_drainage.h, the kernels f3d_drainage.hip) -- the queries f3d_session_drainage (directions,
// accumulation, basins) and f3d_session_streams (the stream network as segments), behind join_bands like the rasters, and the
// update f3d_session_paint_streams, which emits the segments straight into the session's paint buffer and hands them to the
// paint's own count, bin and paint launches (paint_run, f3d_host_paint.h) on the paint's Update path.  Every call routes the
// whole DEM afresh from the tables as they are: nothing is kept between calls, so a re-terrain has nothing to invalidate.
// With F3D_DRAINAGE_FILL the three route over the filled surface (f3d_fill.h, f3d_fill.hip: the fill and flat passes, then
// k_fill_direction in place of k_drain_direction); the query f3d_session_fill returns that surface on its own.
// The order in which refusals win is contract (include/f3d_terrain_pt.h).
#pragma once

#include "f3d_drainage.h"
#include "f3d_fill.h"

namespace {

// The checks the three entries share, after the struct size: flags, reserved, the region of samples.
template <class Desc>
void drain_front(const f3d_session &s, const Desc &q, uint32_t known, const char *names) {
    check_flags(q.flags, known, "drainage", names);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the drainage descriptor's reserved member must be 0, got %u", q.reserved);
    raster_region(s, q, "drainage");
}

// ... and, after an entry's own: a DEM the pointer word cannot index.
void drain_size(const f3d_session &s) {
    const uint64_t n = ((uint64_t)s.params.terrain.cell_w + 1u) * ((uint64_t)s.params.terrain.cell_h + 1u);
    if (n > kDrainMaxSamples)
        fail(F3D_STATUS_VALUE, "drainage routes at most 2^31 samples (the live bit shares the pointer word), the DEM has %llu", (unsigned long long)n);
}

// One kind of counter down (kDrainSlots words) and its slots summed, or maximised.
uint64_t drain_read_back(f3d_session &s, const uint32_t *first, bool sum) {
    uint32_t slots[kDrainSlots];
    hip_check(hipMemcpyAsync(slots, first, sizeof slots, hipMemcpyDeviceToHost, s.stream), "drainage counters");
    hip_check(hipStreamSynchronize(s.stream), "drainage counters");
    uint64_t all = 0u;
    for (uint32_t v : slots) all = sum ? all + v : std::max<uint64_t>(all, v);
    return all;
}

// The fill's scratch: its counters, two planes of dirty flags (a word a tile), then the z, W and T planes --
// kFillBytesPerSample a sample.  fill_place lays it out at `base` (the caller has grown the scratch and joined the bands);
// fill_passes runs the fill pass, then the flat pass, each until the counter read back after a round says that no tile was
// marked for the next.  There is no round cap: every round that marks a tile lowered a value drawn from a finite set.
constexpr uint64_t kFillBytesPerSample = 12u, kDrainFilledBytesPerSample = 33u;
static_assert(kFillBytesPerSample == 2u * sizeof(float) + sizeof(uint32_t), "z, W, T");
size_t fill_bytes(size_t n, uint32_t tiles) {
    return paint_align(kFillCounters * sizeof(uint32_t)) + 2u * paint_align((size_t)tiles * sizeof(uint32_t)) + 3u * paint_align(n * sizeof(uint32_t));
}
void fill_place(const f3d_session &s, FillParams &F, char *base) {
    const TerrainDev &T = s.params.terrain;
    F.terrain = T;
    F.w = T.cell_w + 1u, F.h = T.cell_h + 1u;
    F.tile = kFillTile;
    const size_t n = (size_t)F.w * F.h, plane = paint_align(n * sizeof(uint32_t)), flags = paint_align((size_t)fill_tiles(F.w, F.h, kFillTile) * sizeof(uint32_t));
    F.counters = (uint32_t *)base;
    base += paint_align(kFillCounters * sizeof(uint32_t));
    F.dirty[0] = (uint32_t *)base, F.dirty[1] = (uint32_t *)(base + flags);
    base += 2u * flags;
    F.z = (float *)base, F.W = (float *)(base + plane), F.T = (uint32_t *)(base + 2u * plane);
}
struct FillRan {
    uint32_t rounds[2];  // the fill pass's, the flat pass's
    double ms[2];        // host clock to the device's end of each
};
FillRan fill_passes(f3d_session &s, FillParams &F) {
    FillRan got{{0u, 0u}, {0.0, 0.0}};
    auto t0 = std::chrono::steady_clock::now();
    hip_check(launch_fill_init(F, s.stream), "fill init kernel");
    for (int pass = 0; pass < 2; pass++) {
        uint64_t marked = 1u;  // (the fill pass starts with every tile dirty)
        if (pass == 1) {
            hip_check(launch_flat_init(F, s.stream), "flat init kernel");
            marked = drain_read_back(s, F.counters + kFillMarks, true);
        }
        for (uint32_t r = 0u; marked != 0u; r++) {
            F.round = r;
            hip_check(pass == 0 ? launch_fill_relax(F, s.stream) : launch_flat_relax(F, s.stream), "fill relax kernel");
            marked = drain_read_back(s, F.counters + kFillMarks + ((r + 1u) & 1u) * kDrainSlots, true);
            if (got.rounds[pass] != 0xFFFFFFFFu) got.rounds[pass]++;
        }
        const auto t1 = std::chrono::steady_clock::now();
        got.ms[pass] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
    return got;
}

// Scratch of a call in the rasters' buffer: the counters, the code plane, two pointer planes, two count planes, the depth plane
// -- kDrainBytesPerSample a sample --, with `fill` the fill's scratch behind them -- kDrainFilledBytesPerSample in all --, then
// `extra` bytes of the caller's.  Routes the whole DEM: the direction pass (with `fill`: the fill and flat passes, then the
// direction pass on the filled surface), then doubling rounds until the counter read back after each says that no sample is
// live.  R.q and R.s are the final planes.
constexpr uint64_t kDrainBytesPerSample = 21u;
static_assert(kDrainBytesPerSample == sizeof(uint8_t) + 5u * sizeof(uint32_t), "the figure the ABI header and DESIGN.md state");
static_assert(kDrainFilledBytesPerSample == kDrainBytesPerSample + kFillBytesPerSample, "the figure the ABI header and DESIGN.md state");
struct DrainRouted {
    char *extra;
    uint32_t sinks, rounds, longest;
    double ms[2];  // host clock to the device's end of the direction pass (the fill's passes with it), then of the rounds (tools/drainage_time.py)
};
DrainRouted drain_route(f3d_session &s, DrainParams &R, uint64_t extra_bytes, const char *noun, bool fill) {
    const TerrainDev &T = s.params.terrain;
    R.terrain = T;
    R.w = T.cell_w + 1u, R.h = T.cell_h + 1u;
    R.diag = drain_diag(T.spacing_x, T.spacing_z);
    const size_t n = (size_t)R.w * R.h, plane = paint_align(n * sizeof(uint32_t)), counter_bytes = paint_align(kDrainCounters * sizeof(uint32_t));
    const size_t unfilled = counter_bytes + paint_align(n) + 5u * plane, fixed = unfilled + (fill ? fill_bytes(n, fill_tiles(R.w, R.h, kFillTile)) : 0u);
    grow_scratch(s, s.raster_scratch, s.raster_bytes, fixed + extra_bytes, noun, "the scratch of this call brings", "raster scratch");
    char *base = (char *)s.raster_scratch;
    R.counters = (uint32_t *)base;
    R.code = (uint8_t *)(base + counter_bytes);
    uint32_t *planes = (uint32_t *)(base + counter_bytes + paint_align(n));
    const size_t words = plane / sizeof(uint32_t);
    R.q = planes, R.q_next = planes + words, R.s = planes + 2u * words, R.s_next = planes + 3u * words, R.depth = planes + 4u * words;
    join_bands(s);
    const auto t0 = std::chrono::steady_clock::now();
    if (fill) {
        FillParams F{};
        fill_place(s, F, base + unfilled);
        (void)fill_passes(s, F);
        R.fill_W = F.W, R.fill_T = F.T;
        hip_check(launch_fill_direction(R, s.stream), "filled direction kernel");
    } else {
        hip_check(launch_drain_direction(R, s.stream), "drainage direction kernel");
    }
    auto read_back = [&](uint32_t first, bool sum) { return drain_read_back(s, R.counters + first, sum); };
    const uint64_t sinks = read_back(kDrainSinks, true);
    const auto t1 = std::chrono::steady_clock::now();
    DrainRouted got{base + fixed, (uint32_t)std::min<uint64_t>(sinks, 0xFFFFFFFFu), 0u, 0u, {0.0, 0.0}};
    uint64_t live = n - sinks;
    for (uint32_t k = 0u; live != 0u; k++) {
        if (k >= kDrainMaxRounds) fail(F3D_STATUS_DEVICE, "drainage did not settle in %u rounds: the receivers hold a cycle", k);
        R.round = k;
        hip_check(launch_drain_round(R, s.stream), "drainage round kernels");
        std::swap(R.q, R.q_next);
        std::swap(R.s, R.s_next);
        live = read_back(kDrainLiveAt + (k + 1u) * kDrainSlots, true);
        got.rounds++;
    }
    if (got.rounds != 0u) got.longest = (uint32_t)read_back(kDrainLongest, false);
    got.ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    got.ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    return got;
}

void session_drainage(f3d_session &s, const f3d_session_drainage_desc &q) {
    static_assert(F3D_DRAINAGE_DEVICE_POINTERS == kDevicePointers, "one DEVICE_POINTERS for every family");
    check_struct_size(q, "f3d_session_drainage_desc");
    static_assert(F3D_DRAINAGE_FILL == F3D_STREAMS_FILL && (F3D_DRAINAGE_FILL & (kDevicePointers | 0x40u)) == 0u, "one FILL for the three entries");
    drain_front(s, q, F3D_DRAINAGE_DEVICE_POINTERS | F3D_DRAINAGE_FILL, "4 DEVICE_POINTERS, 8 FILL");
    if (!q.stats) fail(F3D_STATUS_VALUE, "null stats for a drainage call: sinks, rounds and longest are always written");
    const bool device_form = (q.flags & kDevicePointers) != 0u;
    if (device_form && ((((uintptr_t)q.accumulation) | ((uintptr_t)q.basin)) & 3u) != 0u)
        fail(F3D_STATUS_VALUE, "drainage accumulation and basin in device memory must be 4-byte aligned");
    drain_size(s);

    DrainParams R{};
    R.row0 = q.row0, R.col0 = q.col0, R.rows = q.rows, R.cols = q.cols;
    const size_t n = (size_t)q.rows * q.cols;
    // the host form's planes pass through the scratch behind the routing's: direction, then accumulation, then basin
    const size_t dir_bytes = (!device_form && q.direction) ? paint_align(n) : 0u, acc_bytes = (!device_form && q.accumulation) ? paint_align(4u * n) : 0u,
                 basin_bytes = (!device_form && q.basin) ? paint_align(4u * n) : 0u;
    const DrainRouted got = drain_route(s, R, dir_bytes + acc_bytes + basin_bytes, "drainage", (q.flags & F3D_DRAINAGE_FILL) != 0u);
    q.stats[0] = got.sinks, q.stats[1] = got.rounds, q.stats[2] = got.longest;
    if (q.ms) q.ms[0] = got.ms[0], q.ms[1] = got.ms[1];
    if (!q.direction && !q.accumulation && !q.basin) return;
    if (device_form) {
        R.out_direction = q.direction, R.out_accumulation = q.accumulation, R.out_basin = q.basin;
    } else {
        R.out_direction = q.direction ? (uint8_t *)got.extra : nullptr;
        R.out_accumulation = q.accumulation ? (uint32_t *)(got.extra + dir_bytes) : nullptr;
        R.out_basin = q.basin ? (uint32_t *)(got.extra + dir_bytes + acc_bytes) : nullptr;
    }
    hip_check(launch_drain_write(R, s.stream), "drainage write kernel");
    if (!device_form) {
        if (q.direction) download_staged(q.direction, R.out_direction, n, s.stream);
        if (q.accumulation) download_staged(q.accumulation, R.out_accumulation, 4u * n, s.stream);
        if (q.basin) download_staged(q.basin, R.out_basin, 4u * n, s.stream);
    }
    hip_check(hipStreamSynchronize(s.stream), "drainage");
}

// What the two stream entries share, after drain_front: threshold, total.
template <class Desc>
void stream_front(const f3d_session &s, const Desc &q, uint32_t known, const char *names) {
    drain_front(s, q, known, names);
    if (q.threshold == 0u) fail(F3D_STATUS_VALUE, "a stream threshold is an accumulation: at least 1, got 0");
    if (!q.total) fail(F3D_STATUS_VALUE, "null total for a stream call: the number of segments is always written");
}

// Routes, then the count pass and the scan over the region's waves: totals, offsets and the scan's storage lie behind the
// routing's planes, then `extra` bytes (the host form's records).  Returns the number of segments.
struct StreamScratch {
    char *extra;
    uint64_t total;
};
template <class Desc>
StreamScratch stream_count(f3d_session &s, const Desc &q, DrainParams &R, uint64_t extra_bytes, const char *noun) {
    R.row0 = q.row0, R.col0 = q.col0, R.rows = q.rows, R.cols = q.cols;
    R.threshold = q.threshold;
    const uint32_t waves = stream_waves(q.rows, q.cols);
    size_t scan_bytes = 0;
    hip_check(contour_scan_bytes(waves, &scan_bytes), "stream scan storage");
    const size_t word_bytes = paint_align(((size_t)waves + 1u) * sizeof(uint64_t)), fixed = 2u * word_bytes + paint_align(scan_bytes);
    const DrainRouted got = drain_route(s, R, fixed + extra_bytes, noun, (q.flags & F3D_STREAMS_FILL) != 0u);
    R.totals = (uint64_t *)got.extra;
    R.offsets = (const uint64_t *)(got.extra + word_bytes);
    hip_check(launch_stream_count(R, got.extra + 2u * word_bytes, scan_bytes, s.stream), "stream count kernels");
    uint64_t total = 0u;
    hip_check(hipMemcpyAsync(&total, R.offsets + waves, sizeof total, hipMemcpyDeviceToHost, s.stream), "stream segment count");
    hip_check(hipStreamSynchronize(s.stream), "stream segment count");
    return {got.extra + fixed, total};
}

void session_streams(f3d_session &s, const f3d_session_streams_desc &q) {
    static_assert(F3D_STREAMS_DEVICE_POINTERS == kDevicePointers, "one DEVICE_POINTERS for every family");
    check_struct_size(q, "f3d_session_streams_desc");
    stream_front(s, q, F3D_STREAMS_DEVICE_POINTERS | F3D_STREAMS_FILL, "4 DEVICE_POINTERS, 8 FILL");
    if (q.capacity != 0u && !q.segments) fail(F3D_STATUS_VALUE, "null segments for a stream call with room for %llu", (unsigned long long)q.capacity);
    const bool device_form = (q.flags & kDevicePointers) != 0u;
    if (device_form && ((uintptr_t)q.segments & 15u) != 0u) fail(F3D_STATUS_VALUE, "stream segments in device memory must be 16-byte aligned");
    drain_size(s);

    DrainParams R{};
    const bool want_seg = q.segments && q.capacity, want_acc = q.accumulation && q.capacity;
    StreamScratch got = stream_count(s, q, R, 0u, "streams");
    const uint64_t n = std::min<uint64_t>(got.total, q.capacity);
    // the host form's records pass through the scratch behind the counters, sized by what will be written, min(total, capacity),
    // as the contours' are.  A scratch too small for them grows -- another buffer --, and the DEM is routed again there.
    const size_t seg_bytes = want_seg ? paint_align((size_t)n * 16u) : 0u, acc_bytes = want_acc ? paint_align((size_t)n * 4u) : 0u;
    if (!device_form && n != 0u && (uint64_t)(got.extra - (char *)s.raster_scratch) + seg_bytes + acc_bytes > s.raster_bytes) {
        got = stream_count(s, q, R, seg_bytes + acc_bytes, "streams");
        if (std::min<uint64_t>(got.total, q.capacity) != n) fail(F3D_STATUS_DEVICE, "the stream count pass counted %llu segments, then %llu", (unsigned long long)n, (unsigned long long)got.total);
    }
    *q.total = got.total;
    if (n == 0u || (!want_seg && !want_acc)) return;
    R.capacity = n;
    if (device_form) {
        R.segments = q.segments;
        R.stream_accumulation = q.accumulation;
    } else {
        R.segments = want_seg ? (float *)got.extra : nullptr;
        R.stream_accumulation = want_acc ? (uint32_t *)(got.extra + seg_bytes) : nullptr;
    }
    hip_check(launch_stream_emit(R, s.stream), "stream emit kernel");
    if (!device_form) {
        if (want_seg) download_staged(q.segments, R.segments, (size_t)n * 16u, s.stream);
        if (want_acc) download_staged(q.accumulation, R.stream_accumulation, (size_t)n * 4u, s.stream);
    }
    hip_check(hipStreamSynchronize(s.stream), "streams");
}

// The filled surface on its own: the fill and flat passes, the counts, the region out of the planes.
void session_fill(f3d_session &s, const f3d_session_fill_desc &q) {
    static_assert(F3D_FILL_DEVICE_POINTERS == kDevicePointers, "one DEVICE_POINTERS for every family");
    check_struct_size(q, "f3d_session_fill_desc");
    check_flags(q.flags, F3D_FILL_DEVICE_POINTERS, "fill", "4 DEVICE_POINTERS");
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the fill descriptor's reserved member must be 0, got %u", q.reserved);
    raster_region(s, q, "fill");
    const bool device_form = (q.flags & kDevicePointers) != 0u;
    if (device_form && ((((uintptr_t)q.filled) | ((uintptr_t)q.depth) | ((uintptr_t)q.flat_distance)) & 3u) != 0u)
        fail(F3D_STATUS_VALUE, "fill planes in device memory must be 4-byte aligned");
    drain_size(s);

    FillParams F{};
    const size_t n = (size_t)q.rows * q.cols, out_plane = paint_align(4u * n);
    const size_t dem = ((size_t)s.params.terrain.cell_w + 1u) * ((size_t)s.params.terrain.cell_h + 1u);
    const size_t fixed = fill_bytes(dem, fill_tiles(s.params.terrain.cell_w + 1u, s.params.terrain.cell_h + 1u, kFillTile));
    // the host form's planes pass through the scratch behind the fill's: filled, then depth, then the flat distance
    void *const outs[3] = {q.filled, q.depth, q.flat_distance};
    size_t at[3], extra = 0u;
    for (int k = 0; k < 3; k++) at[k] = extra, extra += (!device_form && outs[k]) ? out_plane : 0u;
    grow_scratch(s, s.raster_scratch, s.raster_bytes, fixed + extra, "fill", "the scratch of this call brings", "raster scratch");
    char *base = (char *)s.raster_scratch;
    fill_place(s, F, base);
    join_bands(s);
    const FillRan got = fill_passes(s, F);
    if (q.ms) q.ms[0] = got.ms[0], q.ms[1] = got.ms[1];
    if (q.stats) {
        hip_check(launch_fill_stats(F, s.stream), "fill stats kernel");
        q.stats[0] = (uint32_t)std::min<uint64_t>(drain_read_back(s, F.counters + kFillFilled, true), 0xFFFFFFFFu);
        q.stats[1] = got.rounds[0], q.stats[2] = got.rounds[1];
        q.stats[3] = (uint32_t)drain_read_back(s, F.counters + kFillLargest, false);
    }
    if (!q.filled && !q.depth && !q.flat_distance) return;
    F.row0 = q.row0, F.col0 = q.col0, F.rows = q.rows, F.cols = q.cols;
    char *extra_at = base + fixed;
    F.out_filled = !q.filled ? nullptr : (device_form ? q.filled : (float *)(extra_at + at[0]));
    F.out_depth = !q.depth ? nullptr : (device_form ? q.depth : (float *)(extra_at + at[1]));
    F.out_flat = !q.flat_distance ? nullptr : (device_form ? q.flat_distance : (uint32_t *)(extra_at + at[2]));
    hip_check(launch_fill_write(F, s.stream), "fill write kernel");
    if (!device_form) {
        if (q.filled) download_staged(q.filled, F.out_filled, 4u * n, s.stream);
        if (q.depth) download_staged(q.depth, F.out_depth, 4u * n, s.stream);
        if (q.flat_distance) download_staged(q.flat_distance, F.out_flat, 4u * n, s.stream);
    }
    hip_check(hipStreamSynchronize(s.stream), "fill");
}

void session_paint_streams(f3d_session &s, const f3d_session_paint_streams_desc &q) {
    check_struct_size(q, "f3d_session_paint_streams_desc");
    Update u(s, q.aim.arm, &q.aim, "painted");
    stream_front(s, q, F3D_STREAMS_FILL, "8 FILL");
    f3d_session::Drape &D = s.drape;
    if (!D.buffer) fail(F3D_STATUS_VALUE, "this session has no drape: streams are painted into one (f3d_session_drape gives the canvas)");
    if (!std::isfinite(q.half_width) || q.half_width < 0.0f)
        fail(F3D_STATUS_VALUE, "paint half_width must be finite and >= 0 metres, got %g", (double)q.half_width);
    if (!(q.opacity >= 0.0f && q.opacity <= 1.0f)) fail(F3D_STATUS_VALUE, "paint opacity must lie in [0, 1], got %g", (double)q.opacity);
    drain_size(s);
    const TerrainDev &T = s.params.terrain;
    // (REACH of f3d_paint.h, from the region alone: a segment ends on a sample of the region or on one of its eight neighbours)
    const float reach = kPaintMaxReach * paint_ramp(T.spacing_x, D.record.scale_x, T.spacing_z, D.record.scale_z);
    u.validate([&] {
        for (int c = 0; c < 4; c++)
            if (!(q.rgba[c] >= 0.0f && q.rgba[c] <= 1.0f)) fail(F3D_STATUS_UPLOAD, "paint colours must lie in [0, 1] (RGBA, linear)");  // (NaN compares false)
        const uint32_t c0 = q.col0 ? q.col0 - 1u : 0u, c1 = std::min(q.col0 + q.cols, T.cell_w), r0 = q.row0 ? q.row0 - 1u : 0u, r1 = std::min(q.row0 + q.rows, T.cell_h);
        const float corner[4] = {plane_at(T.origin_x, c0, T.spacing_x), plane_at(T.origin_x, c1, T.spacing_x), plane_at(T.origin_z, r0, T.spacing_z),
                                 plane_at(T.origin_z, r1, T.spacing_z)};
        for (float v : corner)
            if (!(std::fabs(v) <= reach))
                fail(F3D_STATUS_UPLOAD, "the stream region reaches more than %u texels of the drape (%g m) from the terrain's centre: beyond the reach the "
                     "rasteriser's f32 distances are sized for (paint a smaller region)", (unsigned)kPaintMaxReach, (double)reach);
    });

    DrainParams R{};
    const StreamScratch got = stream_count(s, q, R, 0u, "paint");
    if (got.total > F3D_PAINT_MAX_PRIMITIVES)
        fail(F3D_STATUS_VALUE, "a paint call takes at most %u primitives, the streams have %llu segments", F3D_PAINT_MAX_PRIMITIVES,
             (unsigned long long)got.total);
    *q.total = got.total;
    if (got.total > 0u) {
        const uint32_t n = (uint32_t)got.total;
        PaintParams P = paint_params(s, F3D_PAINT_LINES, q.half_width, q.opacity);
        const PaintStorage at = paint_records(s, P, n);
        R.capacity = n;
        R.prims = (PaintPrim *)s.paint.prims;
        for (int c = 0; c < 4; c++) R.rgba[c] = q.rgba[c];
        hip_check(launch_stream_emit(R, s.stream), "stream emit kernel");
        paint_run(s, P, at);
    }
    u.apply();
}

}  // namespace

extern "C" {

int f3d_session_drainage(f3d_session *s, const f3d_session_drainage_desc *desc, char *err, size_t errlen) {
    return contour_entry(s, desc, "drainage", session_drainage, err, errlen);
}

int f3d_session_streams(f3d_session *s, const f3d_session_streams_desc *desc, char *err, size_t errlen) {
    return contour_entry(s, desc, "streams", session_streams, err, errlen);
}

int f3d_session_paint_streams(f3d_session *s, const f3d_session_paint_streams_desc *desc, char *err, size_t errlen) {
    return contour_entry(s, desc, "paint-streams", session_paint_streams, err, errlen);
}

int f3d_session_fill(f3d_session *s, const f3d_session_fill_desc *desc, char *err, size_t errlen) {
    return contour_entry(s, desc, "fill", session_fill, err, errlen);
}

}  // extern "C"
