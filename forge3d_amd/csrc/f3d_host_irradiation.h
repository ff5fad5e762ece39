// f3d_host_irradiation.h -- part of f3d_host.hip (included there once, after the horizon rasters): irradiation rasters on a
// live session (f3d_session_irradiation; the kernel's lane is f3d_irradiation.h) -- the checks, the host form's staged copies
// through the rasters' scratch, the launch.
#pragma once

namespace {

constexpr uint32_t kIrradiationTerrainOnly = 1u, kIrradiationCurved = 2u, kIrradiationDevicePointers = 4u, kIrradiationNoWait = 8u,
                   kIrradiationHorizontal = 16u;

void session_irradiation(f3d_session &s, const f3d_session_irradiation_desc &q) {
    check_struct_size(q, "f3d_session_irradiation_desc");
    if (q.flags & ~(kIrradiationTerrainOnly | kIrradiationCurved | kIrradiationDevicePointers | kIrradiationNoWait | kIrradiationHorizontal))
        fail(F3D_STATUS_VALUE, "unknown irradiation flags 0x%x (1 TERRAIN_ONLY, 2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT, 16 HORIZONTAL)", q.flags);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the irradiation descriptor's reserved member must be 0, got %u", q.reserved);
    const bool device_form = (q.flags & kIrradiationDevicePointers) != 0u;
    if ((q.flags & kIrradiationNoWait) && !device_form)
        fail(F3D_STATUS_VALUE, "NO_WAIT needs DEVICE_POINTERS: results in host memory are there when the call returns");
    const uint32_t dem_w = s.params.terrain.cell_w + 1u, dem_h = s.params.terrain.cell_h + 1u;
    if (q.rows == 0u || q.cols == 0u) fail(F3D_STATUS_VALUE, "empty irradiation region: %u rows x %u columns", q.rows, q.cols);
    if (q.row0 >= dem_h || q.rows > dem_h - q.row0 || q.col0 >= dem_w || q.cols > dem_w - q.col0)
        fail(F3D_STATUS_VALUE, "irradiation region rows [%u, +%u) x columns [%u, +%u) lies outside the %ux%u DEM", q.row0, q.rows, q.col0,
             q.cols, dem_h, dem_w);
    if (!std::isfinite(q.lift)) fail(F3D_STATUS_VALUE, "irradiation lift must be finite");
    if (!q.energy && !q.count && !q.normal)
        fail(F3D_STATUS_VALUE, "an irradiation raster needs an output: energy, count and normal are all null");
    const uint32_t k = q.direction_count;
    if (k == 0u && (q.energy || q.count))
        fail(F3D_STATUS_VALUE, "an irradiation raster without directions answers the normals alone: energy and count need direction_count > 0");
    if (k != 0u && !q.directions) fail(F3D_STATUS_VALUE, "null directions for an irradiation raster of %u", k);
    if (!device_form)  // (a device call's lanes answer such a term 0: f3d_irradiation.h)
        for (uint32_t a = 0; a < k; a++) {
            const float *d = q.directions + 4u * (size_t)a;
            if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2]) || !std::isfinite(d[3]))
                fail(F3D_STATUS_VALUE, "irradiation direction %u has a non-finite component", a);
            if (d[3] < 0.0f) fail(F3D_STATUS_VALUE, "irradiation direction %u has a negative weight", a);
        }

    IrradiationParams R{};
    R.frame = s.params;
    if (q.flags & kIrradiationTerrainOnly) R.frame.mesh.traversal_mode = 3u;  // (what a scene without a mesh carries: the terrain-only kernel)
    R.curved = (q.flags & kIrradiationCurved) ? 1u : 0u;
    R.horizontal = (q.flags & kIrradiationHorizontal) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.lift = q.lift;
    R.direction_count = k;
    const size_t n = (size_t)q.rows * q.cols;
    if (device_form) {
        R.directions = (const float4 *)q.directions;
        R.energy = q.energy;
        R.count = q.count;
        R.normal = q.normal;
        join_bands(s);
        hip_check(launch_irradiation(R, s.stream), "irradiation kernel");
        if (!(q.flags & kIrradiationNoWait)) hip_check(hipStreamSynchronize(s.stream), "irradiation");
        return;
    }
    // host form: the rasters' scratch, grown only for a larger call than any before -- energy first, then count, then the
    // normals, then the directions (16 bytes each)
    const size_t energy_bytes = q.energy ? n * 4u : 0u, count_bytes = q.count ? n * 4u : 0u, normal_bytes = q.normal ? n * 12u : 0u;
    const size_t out_room = (energy_bytes + count_bytes + normal_bytes + 15u) & ~(size_t)15u, direction_bytes = (size_t)k * 16u;
    const uint64_t want = (uint64_t)out_room + direction_bytes;
    if (want > s.raster_bytes) {
        check_budget(s, s.mem.device_bytes - s.raster_bytes + want, "irradiation", "the scratch of this call brings");
        Ledger::Take take{s.mem};
        void *fresh = take((size_t)want, "raster scratch");
        take.commit();
        if (s.raster_scratch) s.mem.free(s.raster_scratch, (size_t)s.raster_bytes);  // (nothing is in flight on it: the host forms are blocking)
        s.raster_scratch = fresh;
        s.raster_bytes = want;
    }
    char *base = (char *)s.raster_scratch;
    if (q.energy) R.energy = (float *)base;
    if (q.count) R.count = (uint32_t *)(base + energy_bytes);
    if (q.normal) R.normal = (float *)(base + energy_bytes + count_bytes);
    if (k != 0u) R.directions = (const float4 *)(base + out_room);
    join_bands(s);
    if (k != 0u) upload_staged(base + out_room, q.directions, direction_bytes, s.stream, true);
    hip_check(launch_irradiation(R, s.stream), "irradiation kernel");
    if (q.energy) download_staged(q.energy, R.energy, energy_bytes, s.stream);
    if (q.count) download_staged(q.count, R.count, count_bytes, s.stream);
    if (q.normal) download_staged(q.normal, R.normal, normal_bytes, s.stream);
    hip_check(hipStreamSynchronize(s.stream), "irradiation");
}

}  // namespace

extern "C" {

int f3d_session_irradiation(f3d_session *s, const f3d_session_irradiation_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "irradiation", session_irradiation, err, errlen);
}

}  // extern "C"
