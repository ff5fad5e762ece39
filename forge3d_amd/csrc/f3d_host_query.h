// f3d_host_query.h -- part of f3d_host.hip (included there once, after the session updates): ray queries on a live session
// (f3d_session_query; the kernel's lane is f3d_query.h) -- the checks, the host form's scratch and staged copies, the launch.
#pragma once

namespace {

constexpr uint32_t kQueryTerrainOnly = F3D_QUERY_TERRAIN_ONLY, kQueryCurved = F3D_QUERY_CURVED;
// The host form's scratch holds, per ray, the widest input (8 f32) and every output (kind, t, normal, position,
// primitive, direction: 12 words) whichever of them the caller asks for: its size is a function of `count` alone.
constexpr size_t kQueryInBytes = 32u, kQueryOutWords = 12u, kQueryRayBytes = kQueryInBytes + 4u * kQueryOutWords;

void session_query(f3d_session &s, const f3d_session_query_desc &q) {
    check_struct_size(q, "f3d_session_query_desc");
    if (q.mode > 2u) fail(F3D_STATUS_VALUE, "query mode must be 0 (closest hit), 1 (occlusion) or 2 (pixels of the current camera), got %u", q.mode);
    check_flags(q.flags, kQueryTerrainOnly | kQueryCurved | kDevicePointers | kNoWait, "query", "1 TERRAIN_ONLY, 2 CURVED, 4 DEVICE_POINTERS, 8 NO_WAIT");
    const bool device_form = check_no_wait(q.flags);
    if ((q.flags & kQueryCurved) && q.mode != 1u)
        fail(F3D_STATUS_VALUE, "CURVED is the sun rays' curvature policy of an occlusion query (mode 1); mode %u traces with curvature off", q.mode);
    if (q.mode == 1u && (q.t || q.normal || q.position || q.primitive || q.direction))
        fail(F3D_STATUS_VALUE, "an occlusion query (mode 1) answers `kind` only: an any-hit walk stops at the first surface it meets, "
             "its t, normal, position and primitive are not the closest hit's");
    if (q.direction && q.mode != 2u) fail(F3D_STATUS_VALUE, "`direction` is an output of the pixel query (mode 2): modes 0 and 1 use the caller's direction as given");
    if (q.count == 0u) return;
    if (!q.rays) fail(F3D_STATUS_VALUE, "null rays for a query of %u", q.count);
    if (q.mode == 2u && !device_form) {  // (a device batch's lanes answer such a pixel as a miss: f3d_query.h)
        const uint32_t *px = (const uint32_t *)q.rays;
        for (uint32_t i = 0; i < q.count; i++)
            if (px[2u * (size_t)i] >= s.width || px[2u * (size_t)i + 1u] >= s.height)
                fail(F3D_STATUS_VALUE, "query pixel %u is (%u, %u): outside the %ux%u image", i, px[2u * (size_t)i], px[2u * (size_t)i + 1u], s.width, s.height);
    }

    QueryParams Q{};
    Q.frame = s.params;
    if (q.flags & kQueryTerrainOnly) Q.frame.mesh.traversal_mode = 3u;  // (what a scene without a mesh carries: the terrain-only kernel)
    Q.mode = q.mode;
    Q.curved = (q.flags & kQueryCurved) ? 1u : 0u;
    Q.count = q.count;
    const size_t n = q.count, in_bytes = n * (q.mode == 2u ? sizeof(uint2) : kQueryInBytes);
    if (device_form) {
        if (q.mode == 2u) Q.pixels = (const uint2 *)q.rays;
        else Q.rays = (const float4 *)q.rays;
        Q.kind = q.kind;
        Q.t = q.t;
        Q.normal = q.normal;
        Q.position = q.position;
        Q.primitive = q.primitive;
        Q.direction = q.direction;
        join_bands(s);
        hip_check(launch_query(Q, s.stream), "query kernel");
        if (!(q.flags & kNoWait)) hip_check(hipStreamSynchronize(s.stream), "query");
        return;
    }
    // host form: the session's scratch, grown only for a larger batch than any before
    grow_scratch(s, s.query_scratch, s.query_bytes, (uint64_t)n * kQueryRayBytes, "ray query", "the scratch of this batch brings", "query scratch");
    char *base = (char *)s.query_scratch;
    uint32_t *out = (uint32_t *)(base + n * kQueryInBytes);  // word offsets per ray: kind 0, t 1, normal 2, position 5, primitive 8, direction 9
    if (q.mode == 2u) Q.pixels = (const uint2 *)base;
    else Q.rays = (const float4 *)base;
    if (q.kind) Q.kind = out;
    if (q.t) Q.t = (float *)(out + n);
    if (q.normal) Q.normal = (float *)(out + 2u * n);
    if (q.position) Q.position = (float *)(out + 5u * n);
    if (q.primitive) Q.primitive = out + 8u * n;
    if (q.direction) Q.direction = (float *)(out + 9u * n);
    join_bands(s);
    upload_staged(base, q.rays, in_bytes, s.stream, true);
    hip_check(launch_query(Q, s.stream), "query kernel");
    if (q.kind) download_staged(q.kind, Q.kind, n * 4u, s.stream);
    if (q.t) download_staged(q.t, Q.t, n * 4u, s.stream);
    if (q.normal) download_staged(q.normal, Q.normal, n * 12u, s.stream);
    if (q.position) download_staged(q.position, Q.position, n * 12u, s.stream);
    if (q.primitive) download_staged(q.primitive, Q.primitive, n * 4u, s.stream);
    if (q.direction) download_staged(q.direction, Q.direction, n * 12u, s.stream);
    hip_check(hipStreamSynchronize(s.stream), "query");  // (a query without outputs is blocking too)
}

}  // namespace

extern "C" {

int f3d_session_query(f3d_session *s, const f3d_session_query_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "query", session_query, err, errlen);
}

}  // extern "C"
