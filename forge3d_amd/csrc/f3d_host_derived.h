// f3d_host_derived.h -- part of f3d_host.hip (included by f3d_host_contour.h and f3d_host_drainage.h, behind the rasters and
// the paint): what the entries derived from the session's own terrain share on the host -- contours, drainage, streams, fill
// and the two paints of derived segments.  The door of their C ABI (derived_entry); the host form's outputs, staged through
// the scratch behind a call's own pieces (staged_carve, staged_bind, staged_download); the path of a call that returns
// records (records_run: count, read back the total, emit); the path of a call that paints them (paint_derived).  A family
// hands in its own checks, its count step and its emit launch; nothing here asks which family called.
#pragma once

#include "f3d_scratch_carve.h"

namespace {

// The door of the derived entries: as update_entry, behind a probe for a device -- a process without one is told so
// (status 4) whatever else it hands in, as the entry points that compute without a session are.
template <class Desc>
int derived_entry(f3d_session *s, const Desc *desc, const char *noun, void (*call)(f3d_session &, const Desc &), char *err, size_t errlen) {
    const int rc = c_abi(err, errlen, [&] {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(F3D_STATUS_DEVICE, "no HIP device available: libf3dhip has no CPU fallback");
    });
    return rc != F3D_STATUS_OK ? rc : update_entry(s, desc, noun, call, err, errlen);
}

// The outputs of a call are a list of raster_output()s (f3d_host_rasters.h: the caller's pointer, the bytes, the member of
// the family's *Params; a null caller is absent, 0 bytes).  Unlike the rasters' segments, which raster_run packs back to back
// from offset 0, these lie behind the call's own pieces and every one starts on a multiple of 256: the list is shared, the
// layout is not.  Host form: staged_carve gives each its place from where the call's own pieces end and returns the bytes
// they take, staged_bind -- the scratch grown, `extra` where the call's own pieces end in it -- names them to the kernel,
// staged_download brings them down in list order after the launch.  Device form: nothing is carved and the caller's
// pointers are bound.  Both forms end in the wait.
template <size_t N>
size_t staged_carve(bool device_form, RasterSegment (&outputs)[N]) {
    Carver c;
    for (RasterSegment &g : outputs) g.at.offset = device_form ? 0u : c.take((size_t)g.at.bytes);
    return c.at;
}
template <size_t N>
void staged_bind(const f3d_session &s, bool device_form, RasterSegment (&outputs)[N], size_t extra) {
    for (RasterSegment &g : outputs) {
        g.at.offset += extra;
        g.bind(g.member, device_form ? g.caller : g.at.bytes ? (char *)s.raster_scratch + g.at.offset : nullptr);
    }
}
template <size_t N>
void staged_download(f3d_session &s, bool device_form, RasterSegment (&outputs)[N], const char *noun) {
    for (RasterSegment &g : outputs)
        if (!device_form && g.at.bytes) download_staged(g.caller, (char *)s.raster_scratch + g.at.offset, (size_t)g.at.bytes, s.stream);
    hip_check(hipStreamSynchronize(s.stream), noun);
}

// What a family's count step answers: where the bytes behind its own pieces begin in the rasters' scratch, and the number of
// records.  The step takes the bytes the caller wants there, sizes the scratch, runs its count pass and the scan and reads
// the total back.
struct Counted {
    size_t extra;
    uint64_t total;
};

// The call that returns records.  `outputs`: the records and their parallel word, `bytes` the size of ONE record, the caller
// null when not wanted.  Count; the host form's records pass through the scratch behind the counters, sized by what will be
// written, min(total, capacity), not by the caller's capacity -- a scratch too small for them grows, another buffer, and
// the count step runs again there; *total; emit; the records down.
template <class Params, class Count, class Emit>
void records_run(f3d_session &s, bool device_form, uint64_t capacity, uint64_t *total, Params &R, RasterSegment (&outputs)[2], const char *noun, const char *plural,
                 Count &&count, Emit &&emit) {
    Counted got = count(0u);
    const uint64_t n = std::min<uint64_t>(got.total, capacity);
    for (RasterSegment &g : outputs) g.at.bytes *= n;
    const size_t staged = staged_carve(device_form, outputs);
    if (!device_form && n != 0u && got.extra + staged > s.raster_bytes) {
        got = count(staged);
        if (std::min<uint64_t>(got.total, capacity) != n)
            fail(F3D_STATUS_DEVICE, "the %s count pass counted %llu segments, then %llu", noun, (unsigned long long)n, (unsigned long long)got.total);
    }
    *total = got.total;
    if (n == 0u || (!outputs[0].caller && !outputs[1].caller)) return;
    R.capacity = n;
    staged_bind(s, device_form, outputs, got.extra);
    emit();
    staged_download(s, device_form, outputs, plural);
}

// The words in which the two paints of derived segments differ.
struct DerivedPaint {
    const char *type, *painted, *noun, *plural;  // "f3d_session_paint_contours_desc", "contour lines", "contour", "contours"
};

// The update that paints derived segments without their leaving the device, on the common tail of the two descriptors
// (total, rgba, half_width, opacity, aim).  `front`: the family's checks behind the Update; `region`: its last refusal, if
// it has one behind the stroke's, then the world x of the region's two border columns and the world z of its two border
// rows -- every segment lies between them; `count`: its count step; `emit`: its emit launch into the paint's records.  The
// order in which refusals win is contract.
template <class Desc, class Params, class Front, class Region, class Count, class Emit>
void paint_derived(f3d_session &s, const Desc &q, const DerivedPaint &words, Params &R, Front &&front, Region &&region, Count &&count, Emit &&emit) {
    check_struct_size(q, words.type);
    Update u(s, q.aim.arm, &q.aim, "painted");
    front();
    const f3d_session::Drape &D = s.drape;
    if (!D.buffer) fail(F3D_STATUS_VALUE, "this session has no drape: %s are painted into one (f3d_session_drape gives the canvas)", words.painted);
    paint_stroke(q.half_width, q.opacity);
    float corner[4];
    region(corner);
    const TerrainDev &T = s.params.terrain;
    // (REACH of f3d_paint.h, from the region alone)
    const float reach = kPaintMaxReach * paint_ramp(T.spacing_x, D.record.scale_x, T.spacing_z, D.record.scale_z);
    u.validate([&] {
        for (int c = 0; c < 4; c++)
            if (!(q.rgba[c] >= 0.0f && q.rgba[c] <= 1.0f)) fail(F3D_STATUS_UPLOAD, "paint colours must lie in [0, 1] (RGBA, linear)");  // (NaN compares false)
        for (float v : corner)
            if (!(std::fabs(v) <= reach))
                fail(F3D_STATUS_UPLOAD, "the %s region reaches more than %u texels of the drape (%g m) from the terrain's centre: beyond the reach the "
                     "rasteriser's f32 distances are sized for (paint a smaller region)", words.noun, (unsigned)kPaintMaxReach, (double)reach);
    });

    const Counted got = count(0u);
    if (got.total > F3D_PAINT_MAX_PRIMITIVES)
        fail(F3D_STATUS_VALUE, "a paint call takes at most %u primitives, the %s have %llu segments", F3D_PAINT_MAX_PRIMITIVES, words.plural,
             (unsigned long long)got.total);
    *q.total = got.total;
    if (got.total > 0u) {
        const uint32_t n = (uint32_t)got.total;
        PaintParams P = paint_params(s, F3D_PAINT_LINES, q.half_width, q.opacity);
        const PaintStorage at = paint_records(s, P, n);
        R.capacity = n;
        R.prims = (PaintPrim *)s.paint.prims;
        for (int c = 0; c < 4; c++) R.rgba[c] = q.rgba[c];
        emit();
        paint_run(s, P, at);
    }
    u.apply();
}

}  // namespace
