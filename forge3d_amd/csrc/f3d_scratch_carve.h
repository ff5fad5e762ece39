// f3d_scratch_carve.h -- where the pieces of a paint, contour, drainage or fill call lie in a session's scratch: plain
// arithmetic, no HIP type (tests/scratch_carve_host compiles it alone), as f3d_raster_scratch.h is for the rasters.  Every piece
// starts on a multiple of 256 bytes: a Carver hands out offsets and advances by the piece's bytes rounded up.  A family's
// layout is ONE function from its counts to its pieces' offsets; the call that sizes the scratch reads the carver's `at`
// behind the last piece, the code that places the pointers reads the same struct.  Behind a call's own pieces lie the
// host form's outputs, carved the same way (f3d_host_derived.h).
//   paint records   records (80 bytes each), counts, offsets (n + 1 words of 8 bytes each), the run counter, the scan's storage
//   paint keys      keys, sorted keys (8 bytes each), the run list (4 bytes a run), the sort's storage
//   count           totals, offsets (groups + 1 words of 8 bytes each), [levels, 4 bytes each], the scan's storage
//                   -- the contours' groups are blocks; the streams' are waves, they have no levels, behind the routing
//   drainage        counters, the code plane (a byte a sample), q, q', s, s', depth (4 bytes a sample each)
//   fill            counters, two planes of dirty flags (4 bytes a tile), z, W, T (4 bytes a sample each)
//                   -- alone (f3d_session_fill) or behind the drainage's pieces (F3D_DRAINAGE_FILL)
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

inline size_t paint_align(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

struct Carver {
    size_t at = 0u;  // behind the last piece: the bytes carved so far
    size_t take(size_t bytes) {
        const size_t piece = at;
        at += paint_align(bytes);
        return piece;
    }
};

struct PaintRecordsLayout {
    size_t records, counts, offsets, run_count, scan;
};
inline PaintRecordsLayout paint_records_layout(Carver &c, size_t n, size_t record_bytes, size_t scan_bytes) {
    PaintRecordsLayout L;
    L.records = c.take(n * record_bytes);
    L.counts = c.take((n + 1u) * sizeof(uint64_t));
    L.offsets = c.take((n + 1u) * sizeof(uint64_t));
    L.run_count = c.take(sizeof(uint32_t));
    L.scan = c.take(scan_bytes);
    return L;
}

struct PaintKeysLayout {
    size_t keys, sorted, runs, sort;
};
inline PaintKeysLayout paint_keys_layout(Carver &c, size_t keys, size_t runs, size_t sort_bytes) {
    PaintKeysLayout L;
    L.keys = c.take(keys * sizeof(uint64_t));
    L.sorted = c.take(keys * sizeof(uint64_t));
    L.runs = c.take(runs * sizeof(uint32_t));
    L.sort = c.take(sort_bytes);
    return L;
}

struct CountLayout {
    size_t totals, offsets, levels, scan;
};
inline CountLayout count_layout(Carver &c, size_t groups, size_t levels, size_t scan_bytes) {
    CountLayout L;
    L.totals = c.take((groups + 1u) * sizeof(uint64_t));
    L.offsets = c.take((groups + 1u) * sizeof(uint64_t));
    L.levels = c.take(levels * sizeof(float));
    L.scan = c.take(scan_bytes);
    return L;
}

struct DrainLayout {
    size_t counters, code, q, q_next, s, s_next, depth;
};
inline DrainLayout drain_layout(Carver &c, size_t samples, size_t counter_words) {
    DrainLayout L;
    L.counters = c.take(counter_words * sizeof(uint32_t));
    L.code = c.take(samples);
    for (size_t *plane : {&L.q, &L.q_next, &L.s, &L.s_next, &L.depth}) *plane = c.take(samples * sizeof(uint32_t));
    return L;
}

struct FillLayout {
    size_t counters, dirty[2], z, W, T;
};
inline FillLayout fill_layout(Carver &c, size_t samples, size_t tiles, size_t counter_words) {
    FillLayout L;
    L.counters = c.take(counter_words * sizeof(uint32_t));
    for (size_t &flags : L.dirty) flags = c.take(tiles * sizeof(uint32_t));
    for (size_t *plane : {&L.z, &L.W, &L.T}) *plane = c.take(samples * sizeof(uint32_t));
    return L;
}
