// f3d_host_clearance.h -- part of f3d_host.hip (included there once, after the irradiation rasters): clearance rasters on a
// live session (f3d_session_clearance; the kernel's lane is f3d_clearance.h) -- the checks, the host form's staged copies
// through the rasters' scratch, the launch.
#pragma once

#include "f3d_clearance.h"

namespace {

constexpr uint32_t kClearanceCurved = 2u, kClearanceDevicePointers = 4u, kClearanceNoWait = 8u;

void session_clearance(f3d_session &s, const f3d_session_clearance_desc &q) {
    check_struct_size(q, "f3d_session_clearance_desc");
    if (q.flags & ~(kClearanceCurved | kClearanceDevicePointers | kClearanceNoWait))
        fail(F3D_STATUS_VALUE, "unknown clearance flags 0x%x (2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT)", q.flags);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the clearance descriptor's reserved member must be 0, got %u", q.reserved);
    const bool device_form = (q.flags & kClearanceDevicePointers) != 0u;
    if ((q.flags & kClearanceNoWait) && !device_form)
        fail(F3D_STATUS_VALUE, "NO_WAIT needs DEVICE_POINTERS: results in host memory are there when the call returns");
    const uint32_t dem_w = s.params.terrain.cell_w + 1u, dem_h = s.params.terrain.cell_h + 1u;
    if (q.rows == 0u || q.cols == 0u) fail(F3D_STATUS_VALUE, "empty clearance region: %u rows x %u columns", q.rows, q.cols);
    if (q.row0 >= dem_h || q.rows > dem_h - q.row0 || q.col0 >= dem_w || q.cols > dem_w - q.col0)
        fail(F3D_STATUS_VALUE, "clearance region rows [%u, +%u) x columns [%u, +%u) lies outside the %ux%u DEM", q.row0, q.rows, q.col0, q.cols,
             dem_h, dem_w);
    if (q.observer_count == 0u) fail(F3D_STATUS_VALUE, "a clearance raster needs at least one observer");
    if (!q.observers) fail(F3D_STATUS_VALUE, "null observers for a clearance raster of %u", q.observer_count);
    if (!q.height && !q.lowest) fail(F3D_STATUS_VALUE, "a clearance raster needs an output: height and lowest are both null");
    const uint32_t k = q.observer_count;
    if (!device_form)  // (a device call's lanes answer such an observer NaN: f3d_clearance.h)
        for (uint32_t a = 0; a < k; a++) {
            const float *ob = q.observers + 4u * (size_t)a;
            if (!std::isfinite(ob[0]) || !std::isfinite(ob[1]) || !std::isfinite(ob[2]) || !std::isfinite(ob[3]))
                fail(F3D_STATUS_VALUE, "clearance observer %u is not a finite (x, y, z, max_distance)", a);
            if (ob[3] < 0.0f) fail(F3D_STATUS_VALUE, "clearance observer %u has a negative maximum distance (0: none)", a);
        }

    ClearanceParams R{};
    R.terrain = s.params.terrain;
    R.curved = (q.flags & kClearanceCurved) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.observer_count = k;
    R.step_cap = clearance_step_cap(R.terrain);
    // (F3D_CLEARANCE_BLOCK=0: A/B switch, a wave owns 64 consecutive samples of the region instead of an 8 x 8 block -- same
    // results; profiles/README.md)
    static const bool rows_footprint = [] {
        const char *e = getenv("F3D_CLEARANCE_BLOCK");
        return e && e[0] == '0';
    }();
    R.block = rows_footprint ? 0u : 1u;
    const size_t n = (size_t)q.rows * q.cols;
    if (device_form) {
        R.observers = (const float4 *)q.observers;
        R.height = q.height;
        R.lowest = q.lowest;
        join_bands(s);
        hip_check(launch_clearance(R, s.stream), "clearance kernel");
        if (!(q.flags & kClearanceNoWait)) hip_check(hipStreamSynchronize(s.stream), "clearance");
        return;
    }
    // host form: the rasters' scratch, grown only for a larger call than any before -- the planes first, then lowest, then
    // the observers (16 bytes each)
    const size_t plane_bytes = q.height ? (size_t)k * n * 4u : 0u, lowest_bytes = q.lowest ? n * 4u : 0u;
    const size_t out_room = (plane_bytes + lowest_bytes + 15u) & ~(size_t)15u, observer_bytes = (size_t)k * 16u;
    const uint64_t want = (uint64_t)out_room + observer_bytes;
    if (want > s.raster_bytes) {
        check_budget(s, s.mem.device_bytes - s.raster_bytes + want, "clearance", "the scratch of this call brings");
        Ledger::Take take{s.mem};
        void *fresh = take((size_t)want, "raster scratch");
        take.commit();
        if (s.raster_scratch) s.mem.free(s.raster_scratch, (size_t)s.raster_bytes);  // (nothing is in flight on it: the host forms are blocking)
        s.raster_scratch = fresh;
        s.raster_bytes = want;
    }
    char *base = (char *)s.raster_scratch;
    if (q.height) R.height = (float *)base;
    if (q.lowest) R.lowest = (float *)(base + plane_bytes);
    R.observers = (const float4 *)(base + out_room);
    join_bands(s);
    upload_staged(base + out_room, q.observers, observer_bytes, s.stream, true);
    hip_check(launch_clearance(R, s.stream), "clearance kernel");
    if (q.height) download_staged(q.height, R.height, plane_bytes, s.stream);
    if (q.lowest) download_staged(q.lowest, R.lowest, lowest_bytes, s.stream);
    hip_check(hipStreamSynchronize(s.stream), "clearance");
}

}  // namespace

extern "C" {

int f3d_session_clearance(f3d_session *s, const f3d_session_clearance_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "clearance", session_clearance, err, errlen);
}

}  // extern "C"
