// f3d_host_raster.h -- part of f3d_host.hip (included there once, after the ray queries): DEM visibility rasters on a live
// session (f3d_session_raster; the kernel's lane is f3d_raster.h) -- the checks, the host form's scratch and staged copies,
// the launch.
#pragma once

namespace {

constexpr uint32_t kRasterTerrainOnly = 1u, kRasterCurved = 2u, kRasterDevicePointers = 4u, kRasterNoWait = 8u, kRasterSessionSun = 16u;

void session_raster(f3d_session &s, const f3d_session_raster_desc &q) {
    check_struct_size(q, "f3d_session_raster_desc");
    if (q.mode > 1u) fail(F3D_STATUS_VALUE, "raster mode must be 0 (toward a point) or 1 (along a direction), got %u", q.mode);
    if (q.flags & ~(kRasterTerrainOnly | kRasterCurved | kRasterDevicePointers | kRasterNoWait | kRasterSessionSun))
        fail(F3D_STATUS_VALUE, "unknown raster flags 0x%x (1 TERRAIN_ONLY, 2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT, 16 SESSION_SUN)", q.flags);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the raster descriptor's reserved member must be 0, got %u", q.reserved);
    const bool device_form = (q.flags & kRasterDevicePointers) != 0u, session_sun = (q.flags & kRasterSessionSun) != 0u;
    if ((q.flags & kRasterNoWait) && !device_form)
        fail(F3D_STATUS_VALUE, "NO_WAIT needs DEVICE_POINTERS: results in host memory are there when the call returns");
    if (session_sun && (q.target_count != 0u || q.targets))
        fail(F3D_STATUS_VALUE, "SESSION_SUN is the session's own sun direction: it takes no targets (got %u)", q.target_count);
    if (session_sun && q.mode != 1u) fail(F3D_STATUS_VALUE, "SESSION_SUN is a direction: it needs mode 1 (along a direction), got mode %u", q.mode);
    const uint32_t dem_w = s.params.terrain.cell_w + 1u, dem_h = s.params.terrain.cell_h + 1u;
    if (q.rows == 0u || q.cols == 0u) fail(F3D_STATUS_VALUE, "empty raster region: %u rows x %u columns", q.rows, q.cols);
    if (q.row0 >= dem_h || q.rows > dem_h - q.row0 || q.col0 >= dem_w || q.cols > dem_w - q.col0)
        fail(F3D_STATUS_VALUE, "raster region rows [%u, +%u) x columns [%u, +%u) lies outside the %ux%u DEM", q.row0, q.rows, q.col0, q.cols,
             dem_h, dem_w);
    if (!std::isfinite(q.lift)) fail(F3D_STATUS_VALUE, "raster lift must be finite");
    if (!q.masks && !q.count) fail(F3D_STATUS_VALUE, "a raster needs an output: masks and count are both null");
    const uint32_t k = session_sun ? 1u : q.target_count;
    if (k == 0u) return;
    if (!session_sun && !q.targets) fail(F3D_STATUS_VALUE, "null targets for a raster of %u", q.target_count);
    if (!session_sun && !device_form)  // (a device call's lanes answer such a target 0: f3d_raster.h)
        for (size_t i = 0; i < 4u * (size_t)k; i++)
            if (!std::isfinite(q.targets[i])) fail(F3D_STATUS_VALUE, "raster target %zu has a non-finite component", i / 4u);

    RasterParams R{};
    R.frame = s.params;
    if (q.flags & kRasterTerrainOnly) R.frame.mesh.traversal_mode = 3u;  // (what a scene without a mesh carries: the terrain-only kernel)
    R.mode = q.mode;
    R.curved = (q.flags & kRasterCurved) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.lift = q.lift;
    R.target_count = k;
    const size_t n = (size_t)q.rows * q.cols, words = (n + 63u) >> 6;
    if (device_form) {
        R.targets = (const float4 *)q.targets;
        R.masks = (unsigned long long *)q.masks;
        R.count = q.count;
        join_bands(s);
        hip_check(launch_raster(R, s.stream), "raster kernel");
        if (!(q.flags & kRasterNoWait)) hip_check(hipStreamSynchronize(s.stream), "raster");
        return;
    }
    // host form: the session's scratch, grown only for a larger call than any before -- masks (8-byte words) first, then the
    // targets (16 bytes each), then count
    const size_t mask_bytes = q.masks ? (size_t)k * words * 8u : 0u, target_bytes = session_sun ? 0u : (size_t)k * 16u;
    const size_t mask_room = (mask_bytes + 15u) & ~(size_t)15u, count_bytes = q.count ? n * 4u : 0u;
    const uint64_t want = (uint64_t)mask_room + target_bytes + count_bytes;
    if (want > s.raster_bytes) {
        check_budget(s, s.mem.device_bytes - s.raster_bytes + want, "raster", "the scratch of this call brings");
        Ledger::Take take{s.mem};
        void *fresh = take((size_t)want, "raster scratch");
        take.commit();
        if (s.raster_scratch) s.mem.free(s.raster_scratch, (size_t)s.raster_bytes);  // (no raster is in flight: the host form is blocking)
        s.raster_scratch = fresh;
        s.raster_bytes = want;
    }
    char *base = (char *)s.raster_scratch;
    if (q.masks) R.masks = (unsigned long long *)base;
    if (!session_sun) R.targets = (const float4 *)(base + mask_room);
    if (q.count) R.count = (uint32_t *)(base + mask_room + target_bytes);
    join_bands(s);
    if (!session_sun) upload_staged(base + mask_room, q.targets, target_bytes, s.stream, true);
    hip_check(launch_raster(R, s.stream), "raster kernel");
    if (q.masks) download_staged(q.masks, R.masks, mask_bytes, s.stream);
    if (q.count) download_staged(q.count, R.count, count_bytes, s.stream);
    hip_check(hipStreamSynchronize(s.stream), "raster");
}

}  // namespace

extern "C" {

int f3d_session_raster(f3d_session *s, const f3d_session_raster_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "raster", session_raster, err, errlen);
}

}  // extern "C"
