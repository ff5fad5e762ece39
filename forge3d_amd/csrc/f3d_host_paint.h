// f3d_host_paint.h -- part of f3d_host.hip (included there once, after the drape): vector features painted into the drape of a
// live session (f3d_session_paint; the lanes' bodies are f3d_paint.h, the kernels f3d_paint.hip) -- the checks, the primitive
// records, the two session buffers, binning and the paint kernel, then the update's own path (Update, f3d_host_update.h): a
// paint is a re-aim over a changed canvas.  Behind it the read-back of the drape (f3d_session_drape_read).
#pragma once

#include "f3d_scratch_carve.h"

namespace {

// The stroke of a call -- f3d_session_paint's and the derived paints' (f3d_host_derived.h).
void paint_stroke(float half_width, float opacity) {
    if (!std::isfinite(half_width) || half_width < 0.0f) fail(F3D_STATUS_VALUE, "paint half_width must be finite and >= 0 metres, got %g", (double)half_width);
    if (!(opacity >= 0.0f && opacity <= 1.0f)) fail(F3D_STATUS_VALUE, "paint opacity must lie in [0, 1], got %g", (double)opacity);
}

// The canvas and the style of a call: everything of PaintParams but the records and the binning's storage.
PaintParams paint_params(const f3d_session &s, uint32_t kind, float half_width, float opacity) {
    const f3d_session::Drape &D = s.drape;
    const TerrainDev &T = s.params.terrain;
    PaintParams P{};
    PaintCanvas &C = P.canvas;
    C.texels = (uint2 *)((char *)D.buffer + sizeof(DrapeDev));
    C.rows = D.rows;
    C.cols = D.cols;
    C.origin_x = T.origin_x, C.origin_z = T.origin_z, C.spacing_x = T.spacing_x, C.spacing_z = T.spacing_z;
    C.scale_x = D.record.scale_x, C.offset_x = D.record.offset_x, C.scale_z = D.record.scale_z, C.offset_z = D.record.offset_z;
    C.ramp = paint_ramp(T.spacing_x, C.scale_x, T.spacing_z, C.scale_z);
    P.kind = kind;
    P.half_width = half_width;
    P.opacity = opacity;
    return P;
}

// first buffer: records, counts, offsets, the run counter, the scan's storage -- known before anything runs.  Names them in P;
// the records themselves are the caller's to put there, on the session stream (an upload: f3d_session_paint; a kernel:
// f3d_session_paint_contours).
struct PaintStorage {
    void *scan_tmp;
    size_t scan_bytes;
};
PaintStorage paint_records(f3d_session &s, PaintParams &P, uint32_t n) {
    f3d_session::Paint &B = s.paint;
    size_t scan_bytes = 0;
    hip_check(paint_scan_bytes(n, &scan_bytes), "paint scan storage");
    Carver c;
    const PaintRecordsLayout L = paint_records_layout(c, n, sizeof(PaintPrim), scan_bytes);
    // (the old buffer may still be read by the previous call's kernels: see the second buffer in paint_run)
    grow_scratch(s, B.prims, B.prim_bytes, c.at, "paint", "the primitive records and the binning's counters bring", "paint primitives");
    char *base = (char *)B.prims;
    P.prims = (const PaintPrim *)(base + L.records);
    P.prim_count = n;
    P.counts = (uint64_t *)(base + L.counts);
    P.offsets = (const uint64_t *)(base + L.offsets);
    P.run_count = (uint32_t *)(base + L.run_count);
    return {base + L.scan, scan_bytes};
}

// The records are on the device (or on their way, on the session stream): count, bin, paint, with the timing marks.
void paint_run(f3d_session &s, PaintParams &P, const PaintStorage &at) {
    f3d_session::Paint &B = s.paint;
    const PaintCanvas &C = P.canvas;
    const uint32_t n = P.prim_count, tiles = paint_tiles_x(C) * paint_tiles_z(C);
    void *scan_tmp = at.scan_tmp;
    const size_t scan_bytes = at.scan_bytes;
    for (hipEvent_t &e : B.mark)
        if (!e) hip_check(hipEventCreate(&e), "paint timing event");
    B.timed = false;
    B.last[0] = n, B.last[1] = B.last[2] = 0u;
    hip_check(hipEventRecord(B.mark[0], s.stream), "paint timing event");
    hip_check(launch_paint_count(P, scan_tmp, scan_bytes, s.stream), "paint count kernels");
    hip_check(hipEventRecord(B.mark[1], s.stream), "paint timing event");
    uint64_t total = 0u;
    hip_check(hipMemcpyAsync(&total, P.offsets + n, sizeof total, hipMemcpyDeviceToHost, s.stream), "paint key count");
    hip_check(hipStreamSynchronize(s.stream), "paint key count");

    if (total > 0u) {
        // second buffer, sized exactly now: keys, sorted keys, the run list, the sort's storage
        if (total > 0xFFFF0000ull)
            fail(F3D_STATUS_RENDER, "paint exceeds the memory budget: %llu (tile, primitive) pairs cannot be listed", (unsigned long long)total);
        P.key_count = (uint32_t)total;
        size_t sort_bytes = 0;
        hip_check(paint_sort_bytes(P.key_count, tiles, &sort_bytes), "paint sort storage");
        Carver c;
        const PaintKeysLayout L = paint_keys_layout(c, (size_t)total, (size_t)std::min<uint64_t>(total, tiles), sort_bytes);
        // (a refusal here leaves the first buffer as it has just grown -- gpu_resource_bytes may have risen -- and everything a
        // render or fingerprint reads as it was.  grow_scratch gives the old buffer back at once although the previous call's k_paint
        // may still read it: Ledger::free ends in the pool's device-wide wait or in hipFree, which waits too; a free path that did
        // not would have to wait for the session stream here first)
        grow_scratch(s, B.keys, B.key_bytes, c.at, "paint", "the (tile, primitive) keys and the storage of their sort bring", "paint keys");
        char *kb = (char *)B.keys;
        P.keys = (uint64_t *)(kb + L.keys);
        P.sorted = (const uint64_t *)(kb + L.sorted);
        P.runs = (uint32_t *)(kb + L.runs);
        hip_check(hipEventRecord(B.mark[2], s.stream), "paint timing event");  // (behind the wait for the key count)
        hip_check(launch_paint_bin(P, tiles, kb + L.sort, sort_bytes, s.stream), "paint binning kernels");
        hip_check(hipEventRecord(B.mark[3], s.stream), "paint timing event");
        uint32_t runs = 0u;
        hip_check(hipMemcpyAsync(&runs, P.run_count, sizeof runs, hipMemcpyDeviceToHost, s.stream), "paint tile count");
        hip_check(hipStreamSynchronize(s.stream), "paint tile count");
        if (runs == 0u || runs > tiles) fail(F3D_STATUS_DEVICE, "paint binning listed %u tiles of %u", runs, tiles);
        join_bands(s);  // (frames of bands on their own streams still sample the canvas)
        hip_check(hipEventRecord(B.mark[4], s.stream), "paint timing event");  // (behind the wait for the tile count)
        hip_check(launch_paint(P, runs, s.stream), "paint kernel");
        hip_check(hipEventRecord(B.mark[5], s.stream), "paint timing event");
        B.last[1] = total, B.last[2] = runs;
        B.timed = true;
    }
}

void session_paint(f3d_session &s, const f3d_session_paint_desc &q) {
    check_struct_size(q, "f3d_session_paint_desc");
    Update u(s, q.aim.arm, &q.aim, "painted");
    f3d_session::Drape &D = s.drape;
    if (!D.buffer) fail(F3D_STATUS_VALUE, "this session has no drape: vector features are painted into one (f3d_session_drape gives the canvas)");
    if (q.flags) fail(F3D_STATUS_VALUE, "unknown paint flags 0x%x (none are defined)", q.flags);
    if (q.primitive > F3D_PAINT_TRIANGLES)
        fail(F3D_STATUS_VALUE, "paint primitive must be 0 (points), 1 (lines) or 2 (triangles), got %u", q.primitive);
    const uint32_t per = q.primitive + 1u;
    if (!q.xz || !q.rgba || q.vertex_count == 0u) fail(F3D_STATUS_VALUE, "paint vertices are empty: xz and rgba hold at least one vertex");
    if (!q.indices || q.index_count == 0u || q.index_count % per != 0u)
        fail(F3D_STATUS_VALUE, "%u indices do not make %s: their count is a positive multiple of %u", q.index_count,
             per == 1u ? "points" : per == 2u ? "line segments" : "triangles", per);
    const uint32_t n = q.index_count / per;
    if (n > F3D_PAINT_MAX_PRIMITIVES) fail(F3D_STATUS_VALUE, "a paint call takes at most %u primitives, got %u", F3D_PAINT_MAX_PRIMITIVES, n);
    for (uint32_t i = 0; i < q.index_count; i++)
        if (q.indices[i] >= q.vertex_count)
            fail(F3D_STATUS_VALUE, "paint index %u is %u, the call has %u vertices", i, q.indices[i], q.vertex_count);
    paint_stroke(q.half_width, q.opacity);
    // (REACH of f3d_paint.h: the coordinates the binning's slacks are sized for)
    const float reach = kPaintMaxReach * paint_ramp(s.params.terrain.spacing_x, D.record.scale_x, s.params.terrain.spacing_z, D.record.scale_z);
    u.validate([&] {
        bool bad_xz = false, bad_rgba = false, far = false;
        for (size_t i = 0; i < (size_t)q.vertex_count * 2u; i++) {
            bad_xz = bad_xz || !std::isfinite(q.xz[i]);
            far = far || !(std::fabs(q.xz[i]) <= reach);
        }
        for (size_t i = 0; i < (size_t)q.vertex_count * 4u; i++) bad_rgba = bad_rgba || !(q.rgba[i] >= 0.0f && q.rgba[i] <= 1.0f);  // (NaN compares false)
        if (bad_xz) fail(F3D_STATUS_UPLOAD, "paint vertices contain non-finite coordinates");
        if (far)
            fail(F3D_STATUS_UPLOAD, "paint vertices lie more than %u texels of the drape (%g m) from the terrain's centre: beyond the reach the "
                 "rasteriser's f32 distances are sized for (clip the geometry to the neighbourhood of the terrain)", (unsigned)kPaintMaxReach, (double)reach);
        if (bad_rgba) fail(F3D_STATUS_UPLOAD, "paint colours must lie in [0, 1] (RGBA, linear)");
    });

    // the records: vertices gathered through the indices, the runs of one feature id numbered
    std::vector<PaintPrim> recs(n);
    uint32_t run = 0u, last_id = 0u;
    for (uint32_t i = 0; i < n; i++) {
        PaintPrim &p = recs[i];
        p = PaintPrim{};
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t v = q.indices[(size_t)i * per + (k < per ? k : per - 1u)];  // (a point: a == b; c repeats the last)
            p.v[2u * k] = q.xz[2u * (size_t)v];
            p.v[2u * k + 1u] = q.xz[2u * (size_t)v + 1u];
            for (uint32_t c = 0; c < 4u; c++) p.c[4u * k + c] = q.rgba[4u * (size_t)v + c];
        }
        const uint32_t id = q.feature ? q.feature[q.indices[(size_t)i * per]] : 0u;
        if (i > 0u && id != last_id) run++;
        last_id = id;
        p.feature = run;
    }

    PaintParams P = paint_params(s, q.primitive, q.primitive == F3D_PAINT_TRIANGLES ? 0.0f : q.half_width, q.opacity);
    const PaintStorage at = paint_records(s, P, n);
    upload_staged(s.paint.prims, recs.data(), (size_t)n * sizeof(PaintPrim), s.stream, true);
    paint_run(s, P, at);
    u.apply();
}

void drape_read(f3d_session &s, const uint32_t *region, float *rgb_out) {
    const f3d_session::Drape &D = s.drape;
    if (!D.buffer) fail(F3D_STATUS_VALUE, "this session has no drape to read");
    if (!rgb_out) fail(F3D_STATUS_VALUE, "null output for the drape's texels");
    const uint32_t row0 = region ? region[0] : 0u, col0 = region ? region[1] : 0u, rows = region ? region[2] : D.rows, cols = region ? region[3] : D.cols;
    if (rows == 0u || cols == 0u || row0 >= D.rows || rows > D.rows - row0 || col0 >= D.cols || cols > D.cols - col0)
        fail(F3D_STATUS_VALUE, "drape region of %ux%u texels at texel (%u, %u) leaves the session's %ux%u drape", rows, cols, row0, col0, D.rows, D.cols);
    join_bands(s);
    std::vector<uint2> host((size_t)rows * D.cols);
    const uint2 *texels = (const uint2 *)((const char *)D.buffer + sizeof(DrapeDev));
    download_staged(host.data(), texels + (size_t)row0 * D.cols, host.size() * sizeof(uint2), s.stream);
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < cols; c++) {
            const uint2 t = host[(size_t)r * D.cols + col0 + c];
            float *o = rgb_out + ((size_t)r * cols + c) * 3u;
            o[0] = drape_half(t.x & 0xFFFFu);
            o[1] = drape_half(t.x >> 16);
            o[2] = drape_half(t.y & 0xFFFFu);
        }
}

}  // namespace

extern "C" {

int f3d_session_paint(f3d_session *s, const f3d_session_paint_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "paint", session_paint, err, errlen);
}

int f3d_session_paint_stats(f3d_session *s, double ms[3], uint64_t counts[3]) {
    if (!s || !s->paint.mark[0]) return 0;
    DeviceGuard g(s->device);
    const f3d_session::Paint &B = s->paint;
    for (int k = 0; k < 3; k++) {
        float t = 0.0f;
        const bool ran = k == 0 || B.timed;
        if (ran && (hipEventSynchronize(B.mark[2 * k + 1]) != hipSuccess || hipEventElapsedTime(&t, B.mark[2 * k], B.mark[2 * k + 1]) != hipSuccess)) return 0;
        if (ms) ms[k] = (double)t;
        if (counts) counts[k] = B.last[k];
    }
    return 1;
}

int f3d_session_drape_read(f3d_session *s, const uint32_t region[4], float *rgb_out, char *err, size_t errlen) {
    return c_abi(err, errlen, [&] {
        DeviceGuard g(checked(s).device);
        drape_read(*s, region, rgb_out);
    });
}

}  // extern "C"
