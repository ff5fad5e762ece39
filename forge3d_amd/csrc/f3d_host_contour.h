// f3d_host_contour.h -- part of f3d_host.hip (included there once, after the paint): contour lines of a live session's terrain
// (the lanes' bodies are f3d_contour.h, the kernels f3d_contour.hip) -- the query f3d_session_contours, behind join_bands like
// the rasters, and the update f3d_session_paint_contours, which emits the segments straight into the session's paint buffer
// and hands them to the paint's own count, bin and paint launches (paint_run, f3d_host_paint.h) on the paint's Update path.
// The order in which refusals win is contract (include/f3d_terrain_pt.h).
#pragma once

#include "f3d_contour.h"
#include "f3d_host_derived.h"

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

// Scratch of a call in the rasters' buffer: the count layout (f3d_scratch_carve.h) with the blocks as groups, then `extra_bytes`
// (the host form's records).  Uploads the levels, runs the count pass and the scan, and returns the number of segments.
template <class Desc>
Counted contour_count(f3d_session &s, const Desc &q, ContourParams &R, uint64_t extra_bytes, const char *noun) {
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
    Carver c;
    const CountLayout L = count_layout(c, blocks, q.level_count, scan_bytes);
    grow_scratch(s, s.raster_scratch, s.raster_bytes, c.at + extra_bytes, noun, "the scratch of this call brings", "raster scratch");
    char *base = (char *)s.raster_scratch;
    R.totals = (uint64_t *)(base + L.totals);
    R.offsets = (const uint64_t *)(base + L.offsets);
    R.levels = (const float *)(base + L.levels);
    join_bands(s);
    upload_staged(base + L.levels, q.levels, (size_t)q.level_count * sizeof(float), s.stream, true);
    hip_check(launch_contour_count(R, base + L.scan, scan_bytes, s.stream), "contour count kernels");
    uint64_t total = 0u;
    hip_check(hipMemcpyAsync(&total, R.offsets + blocks, sizeof total, hipMemcpyDeviceToHost, s.stream), "contour segment count");
    hip_check(hipStreamSynchronize(s.stream), "contour segment count");
    return {c.at, total};
}

void session_contours(f3d_session &s, const f3d_session_contours_desc &q) {
    static_assert(F3D_CONTOUR_DEVICE_POINTERS == kDevicePointers, "one DEVICE_POINTERS for every family");
    check_struct_size(q, "f3d_session_contours_desc");
    contour_front(s, q, F3D_CONTOUR_DEVICE_POINTERS, "4 DEVICE_POINTERS");
    if (q.capacity != 0u && !q.segments) fail(F3D_STATUS_VALUE, "null segments for a contour call with room for %llu", (unsigned long long)q.capacity);
    const bool device_form = (q.flags & kDevicePointers) != 0u;
    if (device_form && ((uintptr_t)q.segments & 15u) != 0u) fail(F3D_STATUS_VALUE, "contour segments in device memory must be 16-byte aligned");

    ContourParams R{};
    RasterSegment outputs[] = {raster_output(q.capacity ? q.segments : nullptr, 16u, R.segments), raster_output(q.capacity ? q.level_index : nullptr, 4u, R.level_index)};
    records_run(s, device_form, q.capacity, q.total, R, outputs, "contour", "contours", [&](uint64_t extra_bytes) { return contour_count(s, q, R, extra_bytes, "contours"); },
                [&] { hip_check(launch_contour_emit(R, s.stream), "contour emit kernel"); });
}

void session_paint_contours(f3d_session &s, const f3d_session_paint_contours_desc &q) {
    const TerrainDev &T = s.params.terrain;
    ContourParams R{};
    paint_derived(
        s, q, {"f3d_session_paint_contours_desc", "contour lines", "contour", "contours"}, R, [&] { contour_front(s, q, 0u, "none are defined"); },
        [&](float corner[4]) {  // (every crossing lies between the region's border lines)
            corner[0] = plane_at(T.origin_x, q.col0, T.spacing_x), corner[1] = plane_at(T.origin_x, q.col0 + q.cols, T.spacing_x);
            corner[2] = plane_at(T.origin_z, q.row0, T.spacing_z), corner[3] = plane_at(T.origin_z, q.row0 + q.rows, T.spacing_z);
        },
        [&](uint64_t extra_bytes) { return contour_count(s, q, R, extra_bytes, "paint"); },
        [&] { hip_check(launch_contour_emit(R, s.stream), "contour emit kernel"); });
}

}  // namespace

extern "C" {

int f3d_session_contours(f3d_session *s, const f3d_session_contours_desc *desc, char *err, size_t errlen) {
    return derived_entry(s, desc, "contours", session_contours, err, errlen);
}

int f3d_session_paint_contours(f3d_session *s, const f3d_session_paint_contours_desc *desc, char *err, size_t errlen) {
    return derived_entry(s, desc, "paint-contours", session_paint_contours, err, errlen);
}

}  // extern "C"
