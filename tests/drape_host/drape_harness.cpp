// tests/drape_host/drape_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_drape_host.py compiles it).
// The drape's lane bodies (f3d_drape.h: drape_sample_at / drape_sample, what the draped frame kernels and the draped resolve
// run per hit; drape_pack_at, what k_drape_pack runs per texel) on the host, and draped FRAMES: the emulator's scene set-up
// (emul_session_create) with the product's own frame bodies instantiated with DRAPE = true -- frame_pixel<true> for one
// sample lane, a mirror of frame_lanes<S, true> for more (the emulator's frame_pixel_lanes with sample_shade<true>), then
// resolve_pixel<true>.  The frames run one lane at a time, as the emulator's own frame loop does: a lane of a frame marches a
// primary, a sun and an IBL ray per sample, each a vote of its own on the device (the branches run one after the other under
// EXEC), and the frame's results do not depend on which lanes share a wave (tests/test_emul_parity.py).
#include <cstddef>

#include "../emul/f3d_emul.cpp"

namespace {

// the emulator's frame_pixel_lanes (the CPU mirror of frame_lanes<S>), shading with the draped sample_shade
template <class Pending>
float drape_frame_pixel_lanes(const FrameParams &P, uint32_t gx, uint32_t gy, uint32_t S, Pending &pend) {
    const FrameHead h = frame_head(P, gx, gy);
    uint32_t stream = h.rng;
    V3 radiance = V3{0.0f, 0.0f, 0.0f};
    Reservoir cand = empty_reservoir();
    const uint32_t group = (1u << S) - 1u;
    for (uint32_t s0 = 0u; s0 < P.spp; s0 += S) {
        const uint32_t n_act = P.spp - s0 < S ? P.spp - s0 : S;
        uint32_t pred = h.centre_hit ? group : 0u;
        uint32_t traced[8];
        PrimaryHit ph[8];
        for (uint32_t j = 0; j < 8u; j++) {
            traced[j] = 0xFFFFFFFFu;
            ph[j].hit.kind = 0u;
            ph[j].rng = 0u;
        }
        for (;;) {
            uint32_t draws[8];
            bool need[8], any = false;
            for (uint32_t j = 0; j < S; j++) {
                draws[j] = 2u * j + 2u * (uint32_t)__builtin_popcount(pred & ((1u << j) - 1u));
                need[j] = j < n_act && draws[j] != traced[j];
                any = any || need[j];
            }
            if (!any) break;
            for (uint32_t j = 0; j < S; j++) {
                if (!need[j]) continue;
                uint32_t st = stream;
                rng_skip(st, draws[j]);
                ph[j] = sample_primary(P, gx, gy, st, pend);
                traced[j] = draws[j];
            }
            pred = 0u;
            for (uint32_t j = 0; j < n_act; j++)
                if (ph[j].hit.kind != 0u) pred |= 1u << j;
        }
        SampleOut o[8];
        for (uint32_t j = 0; j < n_act; j++) {
            uint32_t rng = ph[j].rng;
            o[j] = sample_shade<true>(P, h, ph[j], rng, pend);
        }
        for (uint32_t k = 0; k < n_act; k++) accumulate_sample(cand, radiance, o[k].a, o[k].b, o[k].target_pdf);
        rng_skip(stream, 2u * n_act + 2u * (uint32_t)__builtin_popcount(pred));
    }
    return frame_tail(P, gx, gy, cand, radiance);
}

DrapeDev record_of(const uint64_t *texels, uint32_t rows, uint32_t cols, uint32_t filter, const float *reg) {
    DrapeDev D{};
    D.texels = (const uint2 *)texels;
    D.rows = rows;
    D.cols = cols;
    D.filter = filter;
    D.scale_x = reg[0];
    D.offset_x = reg[1];
    D.scale_z = reg[2];
    D.offset_z = reg[3];
    return D;
}

}  // namespace

// f32 texels (rows x cols x channels) into dst (dst_rows x dst_cols packed texels, 8 bytes each) at (at_row, at_col): k_drape_pack's lanes
extern "C" void drape_pack_run(const float *src, uint32_t rows, uint32_t cols, uint32_t channels, uint64_t *dst, uint32_t dst_cols,
                               uint32_t at_row, uint32_t at_col) {
    DrapePackParams B{};
    B.src = src;
    B.dst = (uint2 *)dst;
    B.rows = rows;
    B.cols = cols;
    B.channels = channels;
    B.dst_cols = dst_cols;
    B.at_row = at_row;
    B.at_col = at_col;
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < cols; c++) drape_pack_at(B, r, c);
}

// the drape at n texel coordinates (tx, tz): out[3 n]
extern "C" void drape_sample_texel_run(const uint64_t *texels, uint32_t rows, uint32_t cols, uint32_t filter, uint32_t n, const float *tx,
                                       const float *tz, float *out) {
    const float reg[4] = {1.0f, 0.0f, 1.0f, 0.0f};
    const DrapeDev D = record_of(texels, rows, cols, filter, reg);
    for (uint32_t i = 0; i < n; i++) {
        const V3 a = drape_sample_at(D, tx[i], tz[i]);
        out[3u * i] = a.x;
        out[3u * i + 1u] = a.y;
        out[3u * i + 2u] = a.z;
    }
}

// the drape under n world points (x, z) of a terrain with frame[4] = origin_x, origin_z, spacing_x, spacing_z: out[3 n],
// coords[2 n] (may be null) = the texel coordinates
extern "C" void drape_sample_world_run(const uint64_t *texels, uint32_t rows, uint32_t cols, uint32_t filter, const float *reg, const float *frame,
                                       uint32_t n, const float *x, const float *z, float *out, float *coords) {
    const DrapeDev D = record_of(texels, rows, cols, filter, reg);
    TerrainDev T{};
    T.origin_x = frame[0];
    T.origin_z = frame[1];
    T.spacing_x = frame[2];
    T.spacing_z = frame[3];
    for (uint32_t i = 0; i < n; i++) {
        const V3 a = drape_sample(D, T, x[i], z[i]);
        out[3u * i] = a.x;
        out[3u * i + 1u] = a.y;
        out[3u * i + 2u] = a.z;
        if (coords) drape_coords(D, T, x[i], z[i], coords[2u * i], coords[2u * i + 1u]);
    }
}

// sizeof and the members' offsets of f3d_session_drape_desc, in the header's order
extern "C" uint32_t drape_desc_layout(uint32_t *out, uint32_t capacity) {
    const uint32_t v[] = {(uint32_t)sizeof(f3d_session_drape_desc),
                          (uint32_t)offsetof(f3d_session_drape_desc, struct_size), (uint32_t)offsetof(f3d_session_drape_desc, flags),
                          (uint32_t)offsetof(f3d_session_drape_desc, image), (uint32_t)offsetof(f3d_session_drape_desc, rows),
                          (uint32_t)offsetof(f3d_session_drape_desc, cols), (uint32_t)offsetof(f3d_session_drape_desc, channels),
                          (uint32_t)offsetof(f3d_session_drape_desc, filter), (uint32_t)offsetof(f3d_session_drape_desc, scale_x),
                          (uint32_t)offsetof(f3d_session_drape_desc, offset_x), (uint32_t)offsetof(f3d_session_drape_desc, scale_z),
                          (uint32_t)offsetof(f3d_session_drape_desc, offset_z), (uint32_t)offsetof(f3d_session_drape_desc, at_row),
                          (uint32_t)offsetof(f3d_session_drape_desc, at_col), (uint32_t)offsetof(f3d_session_drape_desc, aim)};
    const uint32_t n = (uint32_t)(sizeof v / sizeof v[0]);
    for (uint32_t i = 0; i < n && i < capacity; i++) out[i] = v[i];
    return n;
}

// `frames` draped frames of the descriptor's scene and their resolve.  mesh_form: 1 the threaded binary walk, 2 four children
// wide.  lanes: 1 = frame_pixel<true>, 2 / 4 / 8 = the mirror of frame_lanes<S, true>.  info[4] = terrain origin x, origin z,
// spacing x, spacing z.  Returns 0, or 1 when the descriptor was refused.
extern "C" int drape_frames(const f3d_terrain_ref_desc *d, int32_t mesh_form, uint32_t lanes, const uint64_t *texels, uint32_t rows, uint32_t cols,
                            uint32_t filter, const float *reg, uint32_t frames, uint8_t *rgba, float *albedo, float *normal, float *depth,
                            float *info) {
    emul_set_use_bvh(mesh_form == 2 ? 2 : 1);
    const size_t res_n = (size_t)(d->height + 2u * kHaloRows) * d->width;
    std::vector<PackedReservoir> res0(res_n, PackedReservoir{0.0f, 0u, 0.0f, 0.0f}), res1(res0);
    char err[256];
    EmulSession *s = (EmulSession *)emul_session_create(d, 0u, 0u, res0.data(), res1.data(), err, sizeof err);
    emul_set_use_bvh(2);
    if (!s) return 1;
    const DrapeDev D = record_of(texels, rows, cols, filter, reg);
    FrameParams &P = s->P;
    P.drape = &D;
    if (info) {
        info[0] = P.terrain.origin_x;
        info[1] = P.terrain.origin_z;
        info[2] = P.terrain.spacing_x;
        info[3] = P.terrain.spacing_z;
    }
    for (uint32_t f = 0; f < frames; f++) {
        P.frame_index = f;
        P.res_out = s->res[f & 1u];
        P.res_in = s->res[(f & 1u) ^ 1u];
#pragma omp parallel for schedule(dynamic, 1)
        for (long y = (long)P.row_begin; y < (long)P.row_end; y++) {
            ArrayPending pend;
            for (uint32_t x = 0; x < s->width; x++) {
                if (lanes > 1u) (void)drape_frame_pixel_lanes(P, x, (uint32_t)y, lanes, pend);
                else (void)frame_pixel<true>(P, x, (uint32_t)y, pend);
            }
        }
    }
    FrameParams R = P;
    R.res_in = s->res[(frames - 1u) & 1u];
    for (uint32_t y = R.row_begin; y < R.row_end; y++)
        for (uint32_t x = 0; x < s->width; x++) (void)resolve_pixel<true>(R, frames, x, y, rgba, albedo, normal, nullptr, s->depth.data());
    memcpy(depth, s->depth.data(), s->depth.size() * sizeof(float));
    emul_session_destroy(s);
    return 0;
}
