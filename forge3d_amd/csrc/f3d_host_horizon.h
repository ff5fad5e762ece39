// f3d_host_horizon.h -- part of f3d_host.hip (included there once, after the visibility rasters): horizon rasters on a live
// session (f3d_session_horizon; the kernel's lane is f3d_horizon.h) -- the checks, the host form's staged copies through the
// rasters' scratch, the launch.
#pragma once

#include "f3d_horizon.h"

namespace {

constexpr uint32_t kHorizonCurved = 2u, kHorizonDevicePointers = 4u, kHorizonNoWait = 8u;

void session_horizon(f3d_session &s, const f3d_session_horizon_desc &q) {
    check_struct_size(q, "f3d_session_horizon_desc");
    if (q.flags & ~(kHorizonCurved | kHorizonDevicePointers | kHorizonNoWait))
        fail(F3D_STATUS_VALUE, "unknown horizon flags 0x%x (2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT)", q.flags);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the horizon descriptor's reserved member must be 0, got %u", q.reserved);
    const bool device_form = (q.flags & kHorizonDevicePointers) != 0u;
    if ((q.flags & kHorizonNoWait) && !device_form)
        fail(F3D_STATUS_VALUE, "NO_WAIT needs DEVICE_POINTERS: results in host memory are there when the call returns");
    const uint32_t dem_w = s.params.terrain.cell_w + 1u, dem_h = s.params.terrain.cell_h + 1u;
    if (q.rows == 0u || q.cols == 0u) fail(F3D_STATUS_VALUE, "empty horizon region: %u rows x %u columns", q.rows, q.cols);
    if (q.row0 >= dem_h || q.rows > dem_h - q.row0 || q.col0 >= dem_w || q.cols > dem_w - q.col0)
        fail(F3D_STATUS_VALUE, "horizon region rows [%u, +%u) x columns [%u, +%u) lies outside the %ux%u DEM", q.row0, q.rows, q.col0, q.cols,
             dem_h, dem_w);
    if (!std::isfinite(q.lift) || q.lift < 0.0f) fail(F3D_STATUS_VALUE, "horizon lift must be finite and not negative");
    if (q.azimuth_count == 0u || q.azimuth_count > kHorizonMaxAzimuths)
        fail(F3D_STATUS_VALUE, "a horizon raster takes 1 to %u azimuths, got %u", kHorizonMaxAzimuths, q.azimuth_count);
    if (!q.azimuths) fail(F3D_STATUS_VALUE, "null azimuths for a horizon raster of %u", q.azimuth_count);
    if (!q.horizon && !q.sky_view) fail(F3D_STATUS_VALUE, "a horizon raster needs an output: horizon and sky_view are both null");
    const uint32_t k = q.azimuth_count;
    if (!device_form)  // (a device call's lanes answer such an azimuth NaN: f3d_horizon.h)
        for (uint32_t a = 0; a < k; a++) {
            const float dx = q.azimuths[2u * a], dz = q.azimuths[2u * a + 1u];
            if (!std::isfinite(dx) || !std::isfinite(dz) || (dx == 0.0f && dz == 0.0f))
                fail(F3D_STATUS_VALUE, "horizon azimuth %u is not a finite, non-zero (dx, dz)", a);
        }

    HorizonParams R{};
    R.terrain = s.params.terrain;
    R.curved = (q.flags & kHorizonCurved) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.lift = q.lift;
    R.azimuth_count = k;
    R.step_cap = horizon_step_cap(R.terrain);
    // (F3D_HORIZON_BLOCK=1: A/B switch, a wave owns an 8 x 8 block of the region -- same results; profiles/README.md)
    static const bool block = getenv("F3D_HORIZON_BLOCK") != nullptr;
    R.block = block ? 1u : 0u;
    const size_t n = (size_t)q.rows * q.cols;
    if (device_form) {
        R.azimuths = (const float2 *)q.azimuths;
        R.horizon = q.horizon;
        R.sky_view = q.sky_view;
        join_bands(s);
        hip_check(launch_horizon(R, s.stream), "horizon kernel");
        if (!(q.flags & kHorizonNoWait)) hip_check(hipStreamSynchronize(s.stream), "horizon");
        return;
    }
    // host form: the rasters' scratch, grown only for a larger call than any before -- the planes first, then sky_view, then
    // the azimuths (8 bytes each)
    const size_t plane_bytes = q.horizon ? (size_t)k * n * 4u : 0u, sky_bytes = q.sky_view ? n * 4u : 0u;
    const size_t out_room = (plane_bytes + sky_bytes + 15u) & ~(size_t)15u, azimuth_bytes = (size_t)k * 8u;
    const uint64_t want = (uint64_t)out_room + azimuth_bytes;
    if (want > s.raster_bytes) {
        check_budget(s, s.mem.device_bytes - s.raster_bytes + want, "horizon", "the scratch of this call brings");
        Ledger::Take take{s.mem};
        void *fresh = take((size_t)want, "raster scratch");
        take.commit();
        if (s.raster_scratch) s.mem.free(s.raster_scratch, (size_t)s.raster_bytes);  // (nothing is in flight on it: the host forms are blocking)
        s.raster_scratch = fresh;
        s.raster_bytes = want;
    }
    char *base = (char *)s.raster_scratch;
    if (q.horizon) R.horizon = (float *)base;
    if (q.sky_view) R.sky_view = (float *)(base + plane_bytes);
    R.azimuths = (const float2 *)(base + out_room);
    join_bands(s);
    upload_staged(base + out_room, q.azimuths, azimuth_bytes, s.stream, true);
    hip_check(launch_horizon(R, s.stream), "horizon kernel");
    if (q.horizon) download_staged(q.horizon, R.horizon, plane_bytes, s.stream);
    if (q.sky_view) download_staged(q.sky_view, R.sky_view, sky_bytes, s.stream);
    hip_check(hipStreamSynchronize(s.stream), "horizon");
}

}  // namespace

extern "C" {

int f3d_session_horizon(f3d_session *s, const f3d_session_horizon_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "horizon", session_horizon, err, errlen);
}

}  // extern "C"
