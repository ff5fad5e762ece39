// f3d_host_drape.h -- part of f3d_host.hip (included there once, after the session updates): an image draped over the terrain
// of a live session (f3d_session_drape; the lanes' bodies are f3d_drape.h) -- the checks, the buffer, the staged upload, the
// packing kernel, and then the update's own path (Update, f3d_host_update.h): a drape is a re-aim under a new terrain albedo.
#pragma once

namespace {

constexpr uint32_t kDrapeDevicePointers = F3D_DRAPE_DEVICE_POINTERS, kDrapeNoWait = F3D_DRAPE_NO_WAIT, kDrapePatch = F3D_DRAPE_PATCH;
constexpr size_t kDrapeSlabBytes = 8u << 20;  // f32 rows in flight between the staging pair and the packing kernel (host form)

void session_drape(f3d_session &s, const f3d_session_drape_desc &q) {
    check_struct_size(q, "f3d_session_drape_desc");
    Update u(s, q.aim.arm, &q.aim, "draped");
    if (q.flags & ~(kDrapeDevicePointers | kDrapeNoWait | kDrapePatch))
        fail(F3D_STATUS_VALUE, "unknown drape flags 0x%x (4 DEVICE_POINTERS, 8 NO_WAIT, 16 PATCH)", q.flags);
    const bool device_form = check_no_wait(q.flags, "an image in host memory has been read"), patch = (q.flags & kDrapePatch) != 0u;
    f3d_session::Drape &D = s.drape;
    if (q.image) {
        if (s.fd_frames)
            fail(F3D_STATUS_VALUE, "this session renders with frames in flight (k_trace / k_merge), which have no draped form: a drape needs the "
                 "fused frame path (f3d_session_opts.frames_in_flight = 0)");
        if (s.variant % 1000 != 0)
            fail(F3D_STATUS_VALUE, "kernel_variant %d selects a register-budget A/B instantiation of the frame kernel, which has no draped "
                 "form: a drape needs the default budget of the fused frame path", s.variant % 1000);
        if (q.channels != 3u && q.channels != 4u)
            fail(F3D_STATUS_VALUE, "a drape has 3 or 4 channels (RGB, or RGBA with the fourth ignored), got %u", q.channels);
        if (q.rows == 0u || q.cols == 0u || q.rows > F3D_DRAPE_MAX_SIDE || q.cols > F3D_DRAPE_MAX_SIDE)
            fail(F3D_STATUS_VALUE, "a drape holds 1..%u texels a side, got %u rows x %u columns", F3D_DRAPE_MAX_SIDE, q.rows, q.cols);
        if (patch) {
            if (!D.buffer) fail(F3D_STATUS_VALUE, "this session has no drape: a window (PATCH) overwrites part of an existing one");
            if (q.at_row >= D.rows || q.rows > D.rows - q.at_row || q.at_col >= D.cols || q.cols > D.cols - q.at_col)
                fail(F3D_STATUS_VALUE, "drape window of %ux%u texels at texel (%u, %u) leaves the session's %ux%u drape (another size needs the "
                     "whole image)", q.rows, q.cols, q.at_row, q.at_col, D.rows, D.cols);
        } else {
            if (q.at_row != 0u || q.at_col != 0u)
                fail(F3D_STATUS_VALUE, "at_row / at_col (%u, %u) place a window: they need the PATCH flag", q.at_row, q.at_col);
            if (q.filter != F3D_DRAPE_NEAREST && q.filter != F3D_DRAPE_BILINEAR)
                fail(F3D_STATUS_VALUE, "drape filter must be 0 (nearest) or 1 (bilinear), got %u", q.filter);
            const float reg[4] = {q.scale_x, q.offset_x, q.scale_z, q.offset_z};
            for (float v : reg)
                if (!std::isfinite(v)) fail(F3D_STATUS_VALUE, "the drape's registration (scale_x, offset_x, scale_z, offset_z) must be finite");
            if (q.scale_x == 0.0f || q.scale_z == 0.0f) fail(F3D_STATUS_VALUE, "the drape's registration scales must not be zero");
        }
    } else if (patch) {
        fail(F3D_STATUS_VALUE, "a null image removes the drape: it takes no window (PATCH)");
    }
    const size_t texels = q.image ? (size_t)q.rows * q.cols : 0u;
    u.validate([&] {
        if (!q.image || device_form) return;  // (a device image: k_drape_pack stores what the scan would refuse as 0)
        bool bad = false;
        for (size_t i = 0; i < texels; i++)
            for (uint32_t c = 0; c < 3u; c++) {
                const float v = q.image[i * q.channels + c];
                bad = bad || !(v >= 0.0f && v <= kDrapeTexelMax);  // (NaN compares false)
            }
        if (bad) fail(F3D_STATUS_UPLOAD, "drape texels must be finite and >= 0 and at most 65504 (they are stored as binary16)");
    });

    if (!q.image) {  // removal: the undraped kernels again, the buffers back once what reads them has run
        if (D.buffer) {
            join_bands(s);
            s.params.drape = nullptr;
            s.mem.free(D.buffer, (size_t)D.bytes);
            if (D.staging) s.mem.free(D.staging, (size_t)D.staging_bytes);
            s.paint.release(s.mem);  // (f3d_session_paint's buffers go with the canvas)
            D = f3d_session::Drape{};
        }
        u.apply();
        return;
    }

    // the buffer (a 64-byte record + the texels) and, host form, the slab the f32 rows pass through: planned against the
    // budget before anything is taken; a refusal leaves the old drape in place
    const bool keep = D.buffer && (patch || (D.rows == q.rows && D.cols == q.cols));
    const uint64_t want = keep ? D.bytes : (uint64_t)sizeof(DrapeDev) + (uint64_t)texels * sizeof(uint2);
    const size_t row_bytes = (size_t)q.cols * q.channels * sizeof(float);
    const uint32_t slab_rows = (uint32_t)std::max<size_t>(1u, std::min<size_t>(q.rows, kDrapeSlabBytes / row_bytes));
    const uint64_t slab = device_form ? 0u : (uint64_t)slab_rows * row_bytes;
    const bool grow = slab > D.staging_bytes;
    if (!keep || grow) {
        check_budget(s, s.mem.device_bytes - (keep ? 0u : D.bytes) + (keep ? 0u : want) - (grow ? D.staging_bytes : 0u) + (grow ? slab : 0u),
                     "drape", "the drape's texels and the slab its rows are uploaded through bring");
        Ledger::Take take{s.mem};
        void *fresh = keep ? D.buffer : take((size_t)want, "drape texels");
        float *fresh_slab = grow ? (float *)take((size_t)slab, "drape upload slab") : D.staging;
        take.commit();
        join_bands(s);
        if (!keep && D.buffer) s.mem.free(D.buffer, (size_t)D.bytes);  // (the allocator waits for the work that reads it)
        if (grow && D.staging) s.mem.free(D.staging, (size_t)D.staging_bytes);
        D.buffer = fresh;
        D.bytes = want;
        D.staging = fresh_slab;
        if (grow) D.staging_bytes = slab;
    }
    join_bands(s);
    if (!patch) {
        D.rows = q.rows;
        D.cols = q.cols;
        DrapeDev rec{};
        rec.texels = (const uint2 *)((const char *)D.buffer + sizeof(DrapeDev));
        rec.rows = q.rows;
        rec.cols = q.cols;
        rec.scale_x = q.scale_x;
        rec.offset_x = q.offset_x;
        rec.scale_z = q.scale_z;
        rec.offset_z = q.offset_z;
        rec.filter = q.filter;
        D.record = rec;
        upload_staged(D.buffer, &rec, sizeof rec, s.stream, true);
    }
    DrapePackParams B{};
    B.dst = (uint2 *)((char *)D.buffer + sizeof(DrapeDev));
    B.cols = q.cols;
    B.channels = q.channels;
    B.dst_cols = D.cols;
    B.at_col = patch ? q.at_col : 0u;
    if (device_form) {
        B.src = q.image;
        B.rows = q.rows;
        B.at_row = patch ? q.at_row : 0u;
        hip_check(launch_drape_pack(B, s.stream), "drape packing kernel");
    } else {
        for (uint32_t r0 = 0u; r0 < q.rows; r0 += slab_rows) {  // (one stream: slab k + 1 is copied behind the kernel that reads slab k)
            const uint32_t n = std::min(slab_rows, q.rows - r0);
            upload_staged(D.staging, (const char *)q.image + (size_t)r0 * row_bytes, (size_t)n * row_bytes, s.stream, true);
            B.src = D.staging;
            B.rows = n;
            B.at_row = (patch ? q.at_row : 0u) + r0;
            hip_check(launch_drape_pack(B, s.stream), "drape packing kernel");
        }
    }
    s.params.drape = (const DrapeDev *)D.buffer;
    u.apply();
    if (device_form && !(q.flags & kDrapeNoWait)) hip_check(hipStreamSynchronize(s.stream), "drape");
}

}  // namespace

extern "C" {

int f3d_session_drape(f3d_session *s, const f3d_session_drape_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "drape", session_drape, err, errlen);
}

int f3d_session_draped(f3d_session *s, uint32_t info[4]) {
    if (!s || !s->drape.buffer) return 0;
    if (info) {
        info[0] = s->drape.rows;
        info[1] = s->drape.cols;
        info[2] = s->drape.record.filter;
        info[3] = (uint32_t)s->drape.bytes;
    }
    return 1;
}

}  // extern "C"
