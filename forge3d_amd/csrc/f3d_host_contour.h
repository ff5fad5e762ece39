// f3d_host_contour.h -- part of f3d_host.hip (included there once, after the paint): contour lines of a live session's terrain
// (the lanes' bodies are f3d_contour.h, the kernels f3d_contour.hip) -- the query f3d_session_contours, behind join_bands like
// the rasters, and the update f3d_session_paint_contours, which emits the segments straight into the session's paint buffer
// and hands them to the paint's own count, bin and paint launches (paint_run, f3d_host_paint.h) on the paint's Update path.
// The order in which refusals win is contract (include/f3d_terrain_pt.h).
#pragma once

#include "f3d_contour.h"

namespace {

// The checks both entries share, after the struct size: flags, reserved, the region of cells, the levels, total.
template <class Desc>
void contour_front(const f3d_session &s, const Desc &q, uint32_t known, const char *names) {
    check_flags(q.flags, known, "contour", names);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the contour descriptor's reserved member must be 0, got %u", q.reserved);
    const uint32_t cell_w = s.params.terrain.cell_w, cell_h = s.params.terrain.cell_h;
    if (q.rows == 0u || q.cols == 0u) fail(F3D_STATUS_VALUE, "empty contour region: %u rows x %u columns of cells", q.rows, q.cols);
    if (q.row0 >= cell_h || q.rows > cell_h - q.row0 || q.col0 >= cell_w || q.cols > cell_w - q.col0)
        fail(F3D_STATUS_VALUE, "contour region rows [%u, +%u) x columns [%u, +%u) lies outside the %ux%u cell grid", q.row0, q.rows, q.col0, q.cols,
             cell_h, cell_w);
    if (!q.levels || q.level_count == 0u) fail(F3D_STATUS_VALUE, "contour levels are empty: levels holds at least one level");
    if (q.level_count > F3D_CONTOUR_MAX_LEVELS)
        fail(F3D_STATUS_VALUE, "a contour call takes at most %u levels, got %u", F3D_CONTOUR_MAX_LEVELS, q.level_count);
    for (uint32_t k = 0; k < q.level_count; k++) {
        if (!std::isfinite(q.levels[k])) fail(F3D_STATUS_VALUE, "contour level %u is not finite", k);
        if (k > 0u && !(q.levels[k] > q.levels[k - 1u]))
            fail(F3D_STATUS_VALUE, "contour levels must be strictly ascending: level %u is %g after %g", k, (double)q.levels[k], (double)q.levels[k - 1u]);
    }
    if (!q.total) fail(F3D_STATUS_VALUE, "null total for a contour call: the number of segments is always written");
}

// Scratch of a call in the rasters' buffer: totals, offsets, the levels, the scan's storage, then `extra` bytes (the host form's
// records).  Uploads the levels, runs the count pass and the scan, and returns the number of segments.
struct ContourScratch {
    char *extra;
    uint64_t total;
};
template <class Desc>
ContourScratch contour_count(f3d_session &s, const Desc &q, ContourParams &R, uint64_t extra_bytes, const char *noun) {
    static_assert(kContourMaxLevels == F3D_CONTOUR_MAX_LEVELS, "one limit in the header and in the lanes");
    R.terrain = s.params.terrain;
    R.row0 = q.row0, R.col0 = q.col0, R.rows = q.rows, R.cols = q.cols;
    contour_blocks(R);
    R.level_count = q.level_count;
    // (F3D_CONTOUR_CULL=0: A/B switch, every block walks every level -- same results; tools/contour_time.py)
    const char *e = getenv("F3D_CONTOUR_CULL");
    R.cull = (e && e[0] == '0') ? 0u : 1u;
    const uint32_t blocks = R.nbx * R.nbz;
    size_t scan_bytes = 0;
    hip_check(contour_scan_bytes(blocks, &scan_bytes), "contour scan storage");
    const size_t word_bytes = paint_align(((size_t)blocks + 1u) * sizeof(uint64_t)), level_bytes = paint_align((size_t)q.level_count * sizeof(float));
    const size_t fixed = 2u * word_bytes + level_bytes + paint_align(scan_bytes);
    grow_scratch(s, s.raster_scratch, s.raster_bytes, fixed + extra_bytes, noun, "the scratch of this call brings", "raster scratch");
    char *base = (char *)s.raster_scratch;
    R.totals = (uint64_t *)base;
    R.offsets = (const uint64_t *)(base + word_bytes);
    R.levels = (const float *)(base + 2u * word_bytes);
    join_bands(s);
    upload_staged(base + 2u * word_bytes, q.levels, (size_t)q.level_count * sizeof(float), s.stream, true);
    hip_check(launch_contour_count(R, base + 2u * word_bytes + level_bytes, scan_bytes, s.stream), "contour count kernels");
    uint64_t total = 0u;
    hip_check(hipMemcpyAsync(&total, R.offsets + blocks, sizeof total, hipMemcpyDeviceToHost, s.stream), "contour segment count");
    hip_check(hipStreamSynchronize(s.stream), "contour segment count");
    return {base + fixed, total};
}

void session_contours(f3d_session &s, const f3d_session_contours_desc &q) {
    static_assert(F3D_CONTOUR_DEVICE_POINTERS == kDevicePointers, "one DEVICE_POINTERS for every family");
    check_struct_size(q, "f3d_session_contours_desc");
    contour_front(s, q, F3D_CONTOUR_DEVICE_POINTERS, "4 DEVICE_POINTERS");
    if (q.capacity != 0u && !q.segments) fail(F3D_STATUS_VALUE, "null segments for a contour call with room for %llu", (unsigned long long)q.capacity);
    const bool device_form = (q.flags & kDevicePointers) != 0u;
    if (device_form && ((uintptr_t)q.segments & 15u) != 0u) fail(F3D_STATUS_VALUE, "contour segments in device memory must be 16-byte aligned");

    ContourParams R{};
    const bool want_seg = q.segments && q.capacity, want_idx = q.level_index && q.capacity;
    ContourScratch got = contour_count(s, q, R, 0u, "contours");
    const uint64_t n = std::min<uint64_t>(got.total, q.capacity);
    // the host form's records pass through the scratch behind the counters: sized by what will be written, min(total, capacity),
    // not by the caller's capacity.  A scratch too small for them grows -- another buffer --, and the count pass runs again there.
    const size_t seg_bytes = want_seg ? paint_align((size_t)n * 16u) : 0u, idx_bytes = want_idx ? paint_align((size_t)n * 4u) : 0u;
    if (!device_form && n != 0u && (uint64_t)(got.extra - (char *)s.raster_scratch) + seg_bytes + idx_bytes > s.raster_bytes) {
        got = contour_count(s, q, R, seg_bytes + idx_bytes, "contours");
        if (std::min<uint64_t>(got.total, q.capacity) != n) fail(F3D_STATUS_DEVICE, "the contour count pass counted %llu segments, then %llu", (unsigned long long)n, (unsigned long long)got.total);
    }
    *q.total = got.total;
    if (n == 0u || (!want_seg && !want_idx)) return;
    R.capacity = n;
    if (device_form) {
        R.segments = q.segments;
        R.level_index = q.level_index;
    } else {
        R.segments = want_seg ? (float *)got.extra : nullptr;
        R.level_index = want_idx ? (uint32_t *)(got.extra + seg_bytes) : nullptr;
    }
    hip_check(launch_contour_emit(R, s.stream), "contour emit kernel");
    if (!device_form) {
        if (want_seg) download_staged(q.segments, R.segments, (size_t)n * 16u, s.stream);
        if (want_idx) download_staged(q.level_index, R.level_index, (size_t)n * 4u, s.stream);
    }
    hip_check(hipStreamSynchronize(s.stream), "contours");
}

void session_paint_contours(f3d_session &s, const f3d_session_paint_contours_desc &q) {
    check_struct_size(q, "f3d_session_paint_contours_desc");
    Update u(s, q.aim.arm, &q.aim, "painted");
    contour_front(s, q, 0u, "none are defined");
    f3d_session::Drape &D = s.drape;
    if (!D.buffer) fail(F3D_STATUS_VALUE, "this session has no drape: contour lines are painted into one (f3d_session_drape gives the canvas)");
    if (!std::isfinite(q.half_width) || q.half_width < 0.0f)
        fail(F3D_STATUS_VALUE, "paint half_width must be finite and >= 0 metres, got %g", (double)q.half_width);
    if (!(q.opacity >= 0.0f && q.opacity <= 1.0f)) fail(F3D_STATUS_VALUE, "paint opacity must lie in [0, 1], got %g", (double)q.opacity);
    const TerrainDev &T = s.params.terrain;
    // (REACH of f3d_paint.h, from the region alone: every crossing lies between the region's border lines)
    const float reach = kPaintMaxReach * paint_ramp(T.spacing_x, D.record.scale_x, T.spacing_z, D.record.scale_z);
    u.validate([&] {
        for (int c = 0; c < 4; c++)
            if (!(q.rgba[c] >= 0.0f && q.rgba[c] <= 1.0f)) fail(F3D_STATUS_UPLOAD, "paint colours must lie in [0, 1] (RGBA, linear)");  // (NaN compares false)
        const float corner[4] = {plane_at(T.origin_x, q.col0, T.spacing_x), plane_at(T.origin_x, q.col0 + q.cols, T.spacing_x),
                                 plane_at(T.origin_z, q.row0, T.spacing_z), plane_at(T.origin_z, q.row0 + q.rows, T.spacing_z)};
        for (float v : corner)
            if (!(std::fabs(v) <= reach))
                fail(F3D_STATUS_UPLOAD, "the contour region reaches more than %u texels of the drape (%g m) from the terrain's centre: beyond the reach the "
                     "rasteriser's f32 distances are sized for (paint a smaller region)", (unsigned)kPaintMaxReach, (double)reach);
    });

    ContourParams R{};
    const ContourScratch got = contour_count(s, q, R, 0u, "paint");
    if (got.total > F3D_PAINT_MAX_PRIMITIVES)
        fail(F3D_STATUS_VALUE, "a paint call takes at most %u primitives, the contours have %llu segments", F3D_PAINT_MAX_PRIMITIVES,
             (unsigned long long)got.total);
    *q.total = got.total;
    if (got.total > 0u) {
        const uint32_t n = (uint32_t)got.total;
        PaintParams P = paint_params(s, F3D_PAINT_LINES, q.half_width, q.opacity);
        const PaintStorage at = paint_records(s, P, n);
        R.capacity = n;
        R.prims = (PaintPrim *)s.paint.prims;
        for (int c = 0; c < 4; c++) R.rgba[c] = q.rgba[c];
        hip_check(launch_contour_emit(R, s.stream), "contour emit kernel");
        paint_run(s, P, at);
    }
    u.apply();
}

// The door of the two contour entries: as update_entry, behind a probe for a device -- a process without one is told so
// (status 4) whatever else it hands in, as the entry points that compute without a session are.
template <class Desc>
int contour_entry(f3d_session *s, const Desc *desc, const char *noun, void (*call)(f3d_session &, const Desc &), char *err, size_t errlen) {
    const int rc = c_abi(err, errlen, [&] {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(F3D_STATUS_DEVICE, "no HIP device available: libf3dhip has no CPU fallback");
    });
    return rc != F3D_STATUS_OK ? rc : update_entry(s, desc, noun, call, err, errlen);
}

}  // namespace

extern "C" {

int f3d_session_contours(f3d_session *s, const f3d_session_contours_desc *desc, char *err, size_t errlen) {
    return contour_entry(s, desc, "contours", session_contours, err, errlen);
}

int f3d_session_paint_contours(f3d_session *s, const f3d_session_paint_contours_desc *desc, char *err, size_t errlen) {
    return contour_entry(s, desc, "paint-contours", session_paint_contours, err, errlen);
}

}  // extern "C"
