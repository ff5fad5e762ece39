// f3d_host_rasters.h -- part of f3d_host.hip (included there once, after the ray queries): the five raster families of a live
// session -- visibility (f3d_session_raster; the kernel's lane is f3d_raster.h), horizon (f3d_session_horizon; f3d_horizon.h),
// irradiation (f3d_session_irradiation; f3d_irradiation.h), clearance (f3d_session_clearance; f3d_clearance.h), shadow depth
// (f3d_session_umbra; f3d_umbra.h) -- and their C
// ABI: what they share in raster_front (raster_flags) / raster_region / raster_run, what is a family's own in its function.  A family is:
// the shared front checks, its own checks (the order in which refusals win is contract), its *Params, the list of its
// segments, raster_run.
#pragma once

#include "f3d_clearance.h"
#include "f3d_horizon.h"
#include "f3d_raster_scratch.h"
#include "f3d_umbra.h"

namespace {

// The front checks: struct size, then unknown flags, `reserved`, NO_WAIT without DEVICE_POINTERS.  Returns whether the call is
// in the device form.  (The raster's `mode` stands between the struct size and the flags: it calls the two halves itself.)
template <class Desc>
bool raster_flags(const Desc &q, const char *noun, uint32_t known, const char *names) {
    check_flags(q.flags, known, noun, names);
    if (q.reserved != 0u) fail(F3D_STATUS_VALUE, "the %s descriptor's reserved member must be 0, got %u", noun, q.reserved);
    return check_no_wait(q.flags);
}
template <class Desc>
bool raster_front(const Desc &q, const char *type, const char *noun, uint32_t known, const char *names) {
    check_struct_size(q, type);
    return raster_flags(q, noun, known, names);
}

// The region: not empty, inside the DEM.
template <class Desc>
void raster_region(const f3d_session &s, const Desc &q, const char *noun) {
    const uint32_t dem_w = s.params.terrain.cell_w + 1u, dem_h = s.params.terrain.cell_h + 1u;
    if (q.rows == 0u || q.cols == 0u) fail(F3D_STATUS_VALUE, "empty %s region: %u rows x %u columns", noun, q.rows, q.cols);
    if (q.row0 >= dem_h || q.rows > dem_h - q.row0 || q.col0 >= dem_w || q.cols > dem_w - q.col0)
        fail(F3D_STATUS_VALUE, "%s region rows [%u, +%u) x columns [%u, +%u) lies outside the %ux%u DEM", noun, q.row0, q.rows, q.col0, q.cols,
             dem_h, dem_w);
}

// One piece of a call: the caller's pointer -- host memory in the host form, device memory in the device form --, its bytes
// (f3d_raster_scratch.h) and the member of the family's *Params that names it to the kernel.
struct RasterSegment {
    ScratchSegment at;
    void *caller;
    void *member;
    void (*bind)(void *member, void *device);
};
template <class T>
RasterSegment raster_output(void *caller, uint64_t bytes, T *&member) {  // (a null output is absent: 0 bytes, a null member)
    return {{caller ? bytes : 0u, false, 0u}, caller, &member, [](void *m, void *device) { *(T **)m = (T *)device; }};
}
template <class T>
RasterSegment raster_input(const void *caller, uint64_t bytes, const T *&member) {
    return {{bytes, true, 0u}, (void *)caller, &member, [](void *m, void *device) { *(const T **)m = (const T *)device; }};
}

// The call itself, behind every check.  Device form: the caller's pointers as they are, the launch, a wait unless NO_WAIT.
// Host form: the segments laid out in the order given in the session's scratch -- one buffer for the five families, grown
// only for a larger call than any before --, the input up if it has bytes, the launch, the outputs down in the order given,
// a wait.  All of it on the session's stream behind every band launch so far.
template <size_t N, class Launch>
void raster_run(f3d_session &s, uint32_t flags, const char *noun, const char *kernel, RasterSegment (&segments)[N], Launch &&launch) {
    if (flags & kDevicePointers) {
        for (RasterSegment &g : segments) g.bind(g.member, g.caller);
        join_bands(s);
        hip_check(launch(), kernel);
        if (!(flags & kNoWait)) hip_check(hipStreamSynchronize(s.stream), noun);
        return;
    }
    ScratchSegment at[N];
    for (size_t i = 0; i < N; i++) at[i] = segments[i].at;
    grow_scratch(s, s.raster_scratch, s.raster_bytes, scratch_layout(at, N), noun, "the scratch of this call brings", "raster scratch");
    char *base = (char *)s.raster_scratch;
    for (size_t i = 0; i < N; i++) segments[i].bind(segments[i].member, at[i].bytes ? base + at[i].offset : nullptr);
    join_bands(s);
    for (size_t i = 0; i < N; i++)
        if (at[i].input && at[i].bytes) upload_staged(base + at[i].offset, segments[i].caller, (size_t)at[i].bytes, s.stream, true);
    hip_check(launch(), kernel);
    for (size_t i = 0; i < N; i++)
        if (!at[i].input && at[i].bytes) download_staged(segments[i].caller, base + at[i].offset, (size_t)at[i].bytes, s.stream);
    hip_check(hipStreamSynchronize(s.stream), noun);
}

void session_raster(f3d_session &s, const f3d_session_raster_desc &q) {
    check_struct_size(q, "f3d_session_raster_desc");
    if (q.mode > 1u) fail(F3D_STATUS_VALUE, "raster mode must be 0 (toward a point) or 1 (along a direction), got %u", q.mode);
    const bool device_form = raster_flags(q, "raster", F3D_RASTER_TERRAIN_ONLY | F3D_RASTER_CURVED | F3D_RASTER_DEVICE_POINTERS | F3D_RASTER_NO_WAIT | F3D_RASTER_SESSION_SUN,
                                          "1 TERRAIN_ONLY, 2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT, 16 SESSION_SUN");
    const bool session_sun = (q.flags & F3D_RASTER_SESSION_SUN) != 0u;
    if (session_sun && (q.target_count != 0u || q.targets))
        fail(F3D_STATUS_VALUE, "SESSION_SUN is the session's own sun direction: it takes no targets (got %u)", q.target_count);
    if (session_sun && q.mode != 1u) fail(F3D_STATUS_VALUE, "SESSION_SUN is a direction: it needs mode 1 (along a direction), got mode %u", q.mode);
    raster_region(s, q, "raster");
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
    if (q.flags & F3D_RASTER_TERRAIN_ONLY) R.frame.mesh.traversal_mode = 3u;  // (what a scene without a mesh carries: the terrain-only kernel)
    R.mode = q.mode;
    R.curved = (q.flags & F3D_RASTER_CURVED) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.lift = q.lift;
    R.target_count = k;
    const uint64_t n = (uint64_t)q.rows * q.cols, words = (n + 63u) >> 6;
    // masks (8-byte words), then the targets (16 bytes each; none: the session's sun), then count
    RasterSegment segments[] = {raster_output(q.masks, k * words * 8u, R.masks), raster_input(q.targets, session_sun ? 0u : (uint64_t)k * 16u, R.targets),
                                raster_output(q.count, n * 4u, R.count)};
    raster_run(s, q.flags, "raster", "raster kernel", segments, [&] { return launch_raster(R, s.stream); });
}

void session_horizon(f3d_session &s, const f3d_session_horizon_desc &q) {
    const bool device_form = raster_front(q, "f3d_session_horizon_desc", "horizon", F3D_HORIZON_CURVED | F3D_HORIZON_DEVICE_POINTERS | F3D_HORIZON_NO_WAIT,
                                          "2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT");
    raster_region(s, q, "horizon");
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
    R.curved = (q.flags & F3D_HORIZON_CURVED) ? 1u : 0u;
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
    const uint64_t n = (uint64_t)q.rows * q.cols;
    // the planes, then sky_view, then the azimuths (8 bytes each)
    RasterSegment segments[] = {raster_output(q.horizon, k * n * 4u, R.horizon), raster_output(q.sky_view, n * 4u, R.sky_view),
                                raster_input(q.azimuths, (uint64_t)k * 8u, R.azimuths)};
    raster_run(s, q.flags, "horizon", "horizon kernel", segments, [&] { return launch_horizon(R, s.stream); });
}

void session_irradiation(f3d_session &s, const f3d_session_irradiation_desc &q) {
    const bool device_form = raster_front(q, "f3d_session_irradiation_desc", "irradiation",
                                          F3D_IRRADIATION_TERRAIN_ONLY | F3D_IRRADIATION_CURVED | F3D_IRRADIATION_DEVICE_POINTERS | F3D_IRRADIATION_NO_WAIT |
                                              F3D_IRRADIATION_HORIZONTAL,
                                          "1 TERRAIN_ONLY, 2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT, 16 HORIZONTAL");
    raster_region(s, q, "irradiation");
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
    if (q.flags & F3D_IRRADIATION_TERRAIN_ONLY) R.frame.mesh.traversal_mode = 3u;  // (what a scene without a mesh carries: the terrain-only kernel)
    R.curved = (q.flags & F3D_IRRADIATION_CURVED) ? 1u : 0u;
    R.horizontal = (q.flags & F3D_IRRADIATION_HORIZONTAL) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.lift = q.lift;
    R.direction_count = k;
    const uint64_t n = (uint64_t)q.rows * q.cols;
    // energy, then count, then the normals, then the directions (16 bytes each)
    RasterSegment segments[] = {raster_output(q.energy, n * 4u, R.energy), raster_output(q.count, n * 4u, R.count),
                                raster_output(q.normal, n * 12u, R.normal), raster_input(q.directions, (uint64_t)k * 16u, R.directions)};
    raster_run(s, q.flags, "irradiation", "irradiation kernel", segments, [&] { return launch_irradiation(R, s.stream); });
}

void session_clearance(f3d_session &s, const f3d_session_clearance_desc &q) {
    const bool device_form = raster_front(q, "f3d_session_clearance_desc", "clearance",
                                          F3D_CLEARANCE_CURVED | F3D_CLEARANCE_DEVICE_POINTERS | F3D_CLEARANCE_NO_WAIT, "2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT");
    raster_region(s, q, "clearance");
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
    R.curved = (q.flags & F3D_CLEARANCE_CURVED) ? 1u : 0u;
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
    const uint64_t n = (uint64_t)q.rows * q.cols;
    // the planes, then lowest, then the observers (16 bytes each)
    RasterSegment segments[] = {raster_output(q.height, k * n * 4u, R.height), raster_output(q.lowest, n * 4u, R.lowest),
                                raster_input(q.observers, (uint64_t)k * 16u, R.observers)};
    raster_run(s, q.flags, "clearance", "clearance kernel", segments, [&] { return launch_clearance(R, s.stream); });
}

void session_umbra(f3d_session &s, const f3d_session_umbra_desc &q) {
    static_assert(F3D_UMBRA_DEVICE_POINTERS == kDevicePointers && F3D_UMBRA_NO_WAIT == kNoWait, "one DEVICE_POINTERS and one NO_WAIT for every family");
    const bool device_form = raster_front(q, "f3d_session_umbra_desc", "umbra", F3D_UMBRA_CURVED | F3D_UMBRA_DEVICE_POINTERS | F3D_UMBRA_NO_WAIT | F3D_UMBRA_SESSION_SUN,
                                          "2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT, 16 SESSION_SUN");
    const bool session_sun = (q.flags & F3D_UMBRA_SESSION_SUN) != 0u;
    if (session_sun && (q.direction_count != 0u || q.directions))
        fail(F3D_STATUS_VALUE, "SESSION_SUN is the session's own sun direction: it takes no directions (got %u)", q.direction_count);
    raster_region(s, q, "umbra");
    if (!session_sun && q.direction_count == 0u) fail(F3D_STATUS_VALUE, "an umbra raster needs at least one direction, or SESSION_SUN");
    if (!session_sun && !q.directions) fail(F3D_STATUS_VALUE, "null directions for an umbra raster of %u", q.direction_count);
    if (!q.depth && !q.deepest) fail(F3D_STATUS_VALUE, "an umbra raster needs an output: depth and deepest are both null");
    const uint32_t k = session_sun ? 1u : q.direction_count;
    if (!session_sun && !device_form)  // (a device call's lanes answer such a direction NaN: f3d_umbra.h)
        for (uint32_t a = 0; a < k; a++) {
            const float *d = q.directions + 4u * (size_t)a;
            if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2]) || (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) || !(d[3] == 0.0f))
                fail(F3D_STATUS_VALUE, "umbra direction %u is not a finite, non-zero (dx, dy, dz, 0)", a);
        }

    UmbraParams R{};
    R.terrain = s.params.terrain;
    R.curved = (q.flags & F3D_UMBRA_CURVED) ? 1u : 0u;
    R.row0 = q.row0;
    R.col0 = q.col0;
    R.rows = q.rows;
    R.cols = q.cols;
    R.direction_count = k;
    R.step_cap = horizon_step_cap(R.terrain);
    R.sun = s.params.light.wi;  // (what k_raster reads for SESSION_SUN)
    // (F3D_UMBRA_BLOCK=0: A/B switch, a wave owns 64 consecutive samples of the region instead of an 8 x 8 block -- same
    // results; profiles/README.md)
    static const bool rows_footprint = [] {
        const char *e = getenv("F3D_UMBRA_BLOCK");
        return e && e[0] == '0';
    }();
    R.block = rows_footprint ? 0u : 1u;
    const uint64_t n = (uint64_t)q.rows * q.cols;
    // the planes, then deepest, then the directions (16 bytes each; none: the session's sun)
    RasterSegment segments[] = {raster_output(q.depth, k * n * 4u, R.depth), raster_output(q.deepest, n * 4u, R.deepest),
                                raster_input(q.directions, session_sun ? 0u : (uint64_t)k * 16u, R.directions)};
    raster_run(s, q.flags, "umbra", "umbra kernel", segments, [&] { return launch_umbra(R, s.stream); });
}

}  // namespace

extern "C" {

int f3d_session_raster(f3d_session *s, const f3d_session_raster_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "raster", session_raster, err, errlen);
}

int f3d_session_horizon(f3d_session *s, const f3d_session_horizon_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "horizon", session_horizon, err, errlen);
}

int f3d_session_irradiation(f3d_session *s, const f3d_session_irradiation_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "irradiation", session_irradiation, err, errlen);
}

int f3d_session_clearance(f3d_session *s, const f3d_session_clearance_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "clearance", session_clearance, err, errlen);
}

int f3d_session_umbra(f3d_session *s, const f3d_session_umbra_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "umbra", session_umbra, err, errlen);
}

}  // extern "C"
