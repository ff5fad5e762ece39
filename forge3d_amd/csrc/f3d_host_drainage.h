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
#include "f3d_host_derived.h"

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
// kFillBytesPerSample a sample.  fill_carve carves it (fill_layout, f3d_scratch_carve.h) behind what the carver holds -- nothing
// for f3d_session_fill, the routing's pieces for drain_route --, fill_place names the pieces in the scratch once the caller has
// grown it; fill_passes runs the fill pass, then the flat pass, each until the counter read back after a round says that no
// tile was marked for the next.  There is no round cap: every round that marks a tile lowered a value drawn from a finite set.
constexpr uint64_t kFillBytesPerSample = 12u, kDrainFilledBytesPerSample = 33u;
static_assert(kFillBytesPerSample == 2u * sizeof(float) + sizeof(uint32_t), "z, W, T");
FillLayout fill_carve(const f3d_session &s, Carver &c) {
    const uint32_t w = s.params.terrain.cell_w + 1u, h = s.params.terrain.cell_h + 1u;
    return fill_layout(c, (size_t)w * h, fill_tiles(w, h, kFillTile), kFillCounters);
}
void fill_place(const f3d_session &s, FillParams &F, const FillLayout &L) {
    const TerrainDev &T = s.params.terrain;
    F.terrain = T;
    F.w = T.cell_w + 1u, F.h = T.cell_h + 1u;
    F.tile = kFillTile;
    char *base = (char *)s.raster_scratch;
    F.counters = (uint32_t *)(base + L.counters);
    F.dirty[0] = (uint32_t *)(base + L.dirty[0]), F.dirty[1] = (uint32_t *)(base + L.dirty[1]);
    F.z = (float *)(base + L.z), F.W = (float *)(base + L.W), F.T = (uint32_t *)(base + L.T);
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
// (drain_layout, f3d_scratch_carve.h) -- kDrainBytesPerSample a sample --, with `fill` the fill's pieces carved behind them
// (fill_carve) -- kDrainFilledBytesPerSample in all --, then `extra_bytes` of the caller's, which begin at `extra`.  Routes
// the whole DEM: the direction pass (with `fill`: the fill and flat passes, then the direction pass on the filled surface),
// then doubling rounds until the counter read back after each says that no sample is live.  R.q and R.s are the final planes.
constexpr uint64_t kDrainBytesPerSample = 21u;
static_assert(kDrainBytesPerSample == sizeof(uint8_t) + 5u * sizeof(uint32_t), "the figure the ABI header and DESIGN.md state");
static_assert(kDrainFilledBytesPerSample == kDrainBytesPerSample + kFillBytesPerSample, "the figure the ABI header and DESIGN.md state");
struct DrainRouted {
    size_t extra;
    uint32_t sinks, rounds, longest;
    double ms[2];  // host clock to the device's end of the direction pass (the fill's passes with it), then of the rounds (tools/drainage_time.py)
};
DrainRouted drain_route(f3d_session &s, DrainParams &R, uint64_t extra_bytes, const char *noun, bool fill) {
    const TerrainDev &T = s.params.terrain;
    R.terrain = T;
    R.w = T.cell_w + 1u, R.h = T.cell_h + 1u;
    R.diag = drain_diag(T.spacing_x, T.spacing_z);
    const size_t n = (size_t)R.w * R.h;
    Carver c;
    const DrainLayout L = drain_layout(c, n, kDrainCounters);
    const FillLayout filled = fill ? fill_carve(s, c) : FillLayout{};
    grow_scratch(s, s.raster_scratch, s.raster_bytes, c.at + extra_bytes, noun, "the scratch of this call brings", "raster scratch");
    char *base = (char *)s.raster_scratch;
    R.counters = (uint32_t *)(base + L.counters);
    R.code = (uint8_t *)(base + L.code);
    R.q = (uint32_t *)(base + L.q), R.q_next = (uint32_t *)(base + L.q_next);
    R.s = (uint32_t *)(base + L.s), R.s_next = (uint32_t *)(base + L.s_next);
    R.depth = (uint32_t *)(base + L.depth);
    join_bands(s);
    const auto t0 = std::chrono::steady_clock::now();
    if (fill) {
        FillParams F{};
        fill_place(s, F, filled);
        (void)fill_passes(s, F);
        R.fill_W = F.W, R.fill_T = F.T;
        hip_check(launch_fill_direction(R, s.stream), "filled direction kernel");
    } else {
        hip_check(launch_drain_direction(R, s.stream), "drainage direction kernel");
    }
    auto read_back = [&](uint32_t first, bool sum) { return drain_read_back(s, R.counters + first, sum); };
    const uint64_t sinks = read_back(kDrainSinks, true);
    const auto t1 = std::chrono::steady_clock::now();
    DrainRouted got{c.at, (uint32_t)std::min<uint64_t>(sinks, 0xFFFFFFFFu), 0u, 0u, {0.0, 0.0}};
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
    RasterSegment outputs[] = {raster_output(q.direction, n, R.out_direction), raster_output(q.accumulation, 4u * n, R.out_accumulation),
                               raster_output(q.basin, 4u * n, R.out_basin)};
    const DrainRouted got = drain_route(s, R, staged_carve(device_form, outputs), "drainage", (q.flags & F3D_DRAINAGE_FILL) != 0u);
    q.stats[0] = got.sinks, q.stats[1] = got.rounds, q.stats[2] = got.longest;
    if (q.ms) q.ms[0] = got.ms[0], q.ms[1] = got.ms[1];
    if (!q.direction && !q.accumulation && !q.basin) return;
    staged_bind(s, device_form, outputs, got.extra);
    hip_check(launch_drain_write(R, s.stream), "drainage write kernel");
    staged_download(s, device_form, outputs, "drainage");
}

// What the two stream entries share, after drain_front: threshold, total.
template <class Desc>
void stream_front(const f3d_session &s, const Desc &q, uint32_t known, const char *names) {
    drain_front(s, q, known, names);
    if (q.threshold == 0u) fail(F3D_STATUS_VALUE, "a stream threshold is an accumulation: at least 1, got 0");
    if (!q.total) fail(F3D_STATUS_VALUE, "null total for a stream call: the number of segments is always written");
}

// Routes, then the count pass and the scan over the region's waves: the count layout (f3d_scratch_carve.h) with the waves as
// groups and no levels lies behind the routing's pieces, then `extra_bytes` (the host form's records).  Returns the number of
// segments.
template <class Desc>
Counted stream_count(f3d_session &s, const Desc &q, DrainParams &R, uint64_t extra_bytes, const char *noun) {
    R.row0 = q.row0, R.col0 = q.col0, R.rows = q.rows, R.cols = q.cols;
    R.threshold = q.threshold;
    const uint32_t waves = stream_waves(q.rows, q.cols);
    size_t scan_bytes = 0;
    hip_check(contour_scan_bytes(waves, &scan_bytes), "stream scan storage");
    Carver c;
    const CountLayout L = count_layout(c, waves, 0u, scan_bytes);
    const DrainRouted got = drain_route(s, R, c.at + extra_bytes, noun, (q.flags & F3D_STREAMS_FILL) != 0u);
    char *base = (char *)s.raster_scratch + got.extra;
    R.totals = (uint64_t *)(base + L.totals);
    R.offsets = (const uint64_t *)(base + L.offsets);
    hip_check(launch_stream_count(R, base + L.scan, scan_bytes, s.stream), "stream count kernels");
    uint64_t total = 0u;
    hip_check(hipMemcpyAsync(&total, R.offsets + waves, sizeof total, hipMemcpyDeviceToHost, s.stream), "stream segment count");
    hip_check(hipStreamSynchronize(s.stream), "stream segment count");
    return {got.extra + c.at, total};
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
    RasterSegment outputs[] = {raster_output(q.capacity ? q.segments : nullptr, 16u, R.segments),
                               raster_output(q.capacity ? q.accumulation : nullptr, 4u, R.stream_accumulation)};
    // (a second count step routes the DEM again in the grown scratch)
    records_run(s, device_form, q.capacity, q.total, R, outputs, "stream", "streams", [&](uint64_t extra_bytes) { return stream_count(s, q, R, extra_bytes, "streams"); },
                [&] { hip_check(launch_stream_emit(R, s.stream), "stream emit kernel"); });
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
    const size_t n = (size_t)q.rows * q.cols;
    // the host form's planes pass through the scratch behind the fill's: filled, then depth, then the flat distance
    RasterSegment outputs[] = {raster_output(q.filled, 4u * n, F.out_filled), raster_output(q.depth, 4u * n, F.out_depth),
                               raster_output(q.flat_distance, 4u * n, F.out_flat)};
    Carver c;
    const FillLayout L = fill_carve(s, c);
    grow_scratch(s, s.raster_scratch, s.raster_bytes, c.at + staged_carve(device_form, outputs), "fill", "the scratch of this call brings", "raster scratch");
    fill_place(s, F, L);
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
    staged_bind(s, device_form, outputs, c.at);
    hip_check(launch_fill_write(F, s.stream), "fill write kernel");
    staged_download(s, device_form, outputs, "fill");
}

void session_paint_streams(f3d_session &s, const f3d_session_paint_streams_desc &q) {
    const TerrainDev &T = s.params.terrain;
    DrainParams R{};
    paint_derived(
        s, q, {"f3d_session_paint_streams_desc", "streams", "stream", "streams"}, R, [&] { stream_front(s, q, F3D_STREAMS_FILL, "8 FILL"); },
        [&](float corner[4]) {  // (a segment ends on a sample of the region or on one of its eight neighbours)
            drain_size(s);
            const uint32_t c0 = q.col0 ? q.col0 - 1u : 0u, c1 = std::min(q.col0 + q.cols, T.cell_w), r0 = q.row0 ? q.row0 - 1u : 0u, r1 = std::min(q.row0 + q.rows, T.cell_h);
            corner[0] = plane_at(T.origin_x, c0, T.spacing_x), corner[1] = plane_at(T.origin_x, c1, T.spacing_x);
            corner[2] = plane_at(T.origin_z, r0, T.spacing_z), corner[3] = plane_at(T.origin_z, r1, T.spacing_z);
        },
        [&](uint64_t extra_bytes) { return stream_count(s, q, R, extra_bytes, "paint"); },
        [&] { hip_check(launch_stream_emit(R, s.stream), "stream emit kernel"); });
}

}  // namespace

extern "C" {

int f3d_session_drainage(f3d_session *s, const f3d_session_drainage_desc *desc, char *err, size_t errlen) {
    return derived_entry(s, desc, "drainage", session_drainage, err, errlen);
}

int f3d_session_streams(f3d_session *s, const f3d_session_streams_desc *desc, char *err, size_t errlen) {
    return derived_entry(s, desc, "streams", session_streams, err, errlen);
}

int f3d_session_paint_streams(f3d_session *s, const f3d_session_paint_streams_desc *desc, char *err, size_t errlen) {
    return derived_entry(s, desc, "paint-streams", session_paint_streams, err, errlen);
}

int f3d_session_fill(f3d_session *s, const f3d_session_fill_desc *desc, char *err, size_t errlen) {
    return derived_entry(s, desc, "fill", session_fill, err, errlen);
}

}  // extern "C"
