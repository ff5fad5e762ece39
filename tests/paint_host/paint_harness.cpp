// tests/paint_host/paint_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_paint_host.py compiles it).
// The lane bodies of f3d_paint.h on the host: paint_texel (every primitive for every texel, no tiles -- the bits the device must
// return), the same texels through the device's tiling (paint_bin's lists, paint_visit over a tile's list only), the coverage and
// the inside decision of one primitive, the tiles paint_bin lists, and the layout of f3d_session_paint_desc.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../forge3d_amd/csrc/f3d_paint.h"
#include "../../include/f3d_terrain_pt.h"

using namespace f3d;

namespace {

// frame[8] = origin_x, origin_z, spacing_x, spacing_z, scale_x, offset_x, scale_z, offset_z
PaintCanvas canvas_of(uint64_t *texels, uint32_t rows, uint32_t cols, const float *frame) {
    PaintCanvas C{};
    C.texels = (uint2 *)texels;
    C.rows = rows;
    C.cols = cols;
    C.origin_x = frame[0], C.origin_z = frame[1], C.spacing_x = frame[2], C.spacing_z = frame[3];
    C.scale_x = frame[4], C.offset_x = frame[5], C.scale_z = frame[6], C.offset_z = frame[7];
    C.ramp = paint_ramp(C.spacing_x, C.scale_x, C.spacing_z, C.scale_z);
    return C;
}

}  // namespace

extern "C" float paint_ramp_run(const float *frame) { return paint_ramp(frame[2], frame[4], frame[3], frame[6]); }

// the texel centres: out[rows][cols][2] = x, z
extern "C" void paint_centres_run(uint32_t rows, uint32_t cols, const float *frame, float *out) {
    const PaintCanvas C = canvas_of(nullptr, rows, cols, frame);
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < cols; c++) paint_centre(C, r, c, out[2u * ((size_t)r * cols + c)], out[2u * ((size_t)r * cols + c) + 1u]);
}

// one call on the host: texels (rows x cols, packed) -> out.  tiled = 0: paint_texel; 1: the device's walk -- per 16 x 16 tile
// the primitives paint_bin lists for it, in primitive order, through paint_visit
extern "C" void paint_run(const uint64_t *texels, uint32_t rows, uint32_t cols, const float *frame, const void *prims, uint32_t n, uint32_t kind,
                          float half_width, float opacity, uint32_t tiled, uint64_t *out, float *values /* untiled only; may be null: f32 RGB before packing */) {
    PaintParams P{};
    P.canvas = canvas_of(const_cast<uint64_t *>(texels), rows, cols, frame);
    P.prims = (const PaintPrim *)prims;
    P.prim_count = n;
    P.kind = kind;
    P.half_width = half_width;
    P.opacity = opacity;
    const PaintCanvas &C = P.canvas;
    if (!tiled) {
#pragma omp parallel for schedule(dynamic, 1)
        for (long r = 0; r < (long)rows; r++)
            for (uint32_t c = 0; c < cols; c++) {
                const uint2 t = paint_texel(P, (uint32_t)r, c);
                out[(size_t)r * cols + c] = (uint64_t)t.x | (uint64_t)t.y << 32;
                if (values) {
                    const V3 v = paint_texel_value(P, (uint32_t)r, c);
                    float *o = values + 3u * ((size_t)r * cols + c);
                    o[0] = v.x, o[1] = v.y, o[2] = v.z;
                }
            }
        return;
    }
    const uint32_t tiles_x = paint_tiles_x(C), tiles = tiles_x * paint_tiles_z(C);
    std::vector<std::vector<uint32_t>> lists(tiles);
    for (uint32_t i = 0; i < n; i++) paint_bin(C, P.prims[i], kind, half_width, [&](uint32_t tile) { lists[tile].push_back(i); });
    for (size_t i = 0; i < (size_t)rows * cols; i++) out[i] = texels[i];
    for (uint32_t tile = 0; tile < tiles; tile++) {
        if (lists[tile].empty()) continue;  // (an empty tile launches nothing)
        for (uint32_t k = 0; k < kPaintTile * kPaintTile; k++) {
            const uint32_t c = (tile % tiles_x) * kPaintTile + (k & (kPaintTile - 1u)), r = (tile / tiles_x) * kPaintTile + k / kPaintTile;
            if (r >= rows || c >= cols) continue;
            const uint2 t = C.texels[(size_t)r * cols + c];
            PaintLane L;
            float x, z;
            paint_centre(C, r, c, x, z);
            paint_begin(L, x, z, V3{drape_half(t.x & 0xFFFFu), drape_half(t.x >> 16), drape_half(t.y & 0xFFFFu)});
            for (uint32_t i : lists[tile]) paint_visit(L, P.prims[i], kind, half_width, C.ramp, opacity);
            const V3 v = paint_end(L, opacity);
            const uint2 o = drape_pack_texel(v.x, v.y, v.z);
            out[(size_t)r * cols + c] = (uint64_t)o.x | (uint64_t)o.y << 32;
        }
    }
}

// one primitive at every texel centre: cov[rows][cols] (a triangle: 1 or 0) and par[rows][cols][2] = (t, 0) of a segment,
// (b1, b2) of a triangle (0 outside)
extern "C" void paint_cov_run(uint32_t rows, uint32_t cols, const float *frame, const void *prim, uint32_t kind, float half_width, float *cov,
                              float *par) {
    const PaintCanvas C = canvas_of(nullptr, rows, cols, frame);
    const PaintPrim &p = *(const PaintPrim *)prim;
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < cols; c++) {
            const size_t i = (size_t)r * cols + c;
            float x, z, a = 0.0f, b = 0.0f;
            paint_centre(C, r, c, x, z);
            if (kind == kPaintTriangles) cov[i] = paint_triangle_in(p, x, z, a, b) ? 1.0f : 0.0f;
            else cov[i] = paint_segment_cov(p, half_width, C.ramp, x, z, a);
            par[2u * i] = a;
            par[2u * i + 1u] = b;
        }
}

// the tiles paint_bin lists for n primitives: counts[n], and the tiles themselves, primitive after primitive, into tiles_out
// (capacity words; returns the number listed, which may exceed the capacity: nothing is written behind it)
extern "C" uint64_t paint_bin_run(uint32_t rows, uint32_t cols, const float *frame, const void *prims, uint32_t n, uint32_t kind, float half_width,
                                  uint32_t *counts, uint32_t *tiles_out, uint64_t capacity) {
    const PaintCanvas C = canvas_of(nullptr, rows, cols, frame);
    const PaintPrim *p = (const PaintPrim *)prims;
    uint64_t total = 0u;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t k = 0u;
        paint_bin(C, p[i], kind, half_width, [&](uint32_t tile) {
            if (total < capacity) tiles_out[total] = tile;
            total++;
            k++;
        });
        counts[i] = k;
    }
    return total;
}

// sizeof and the members' offsets of f3d_session_paint_desc, in the header's order; then sizeof(PaintPrim) and the tile / chunk sizes
extern "C" uint32_t paint_desc_layout(uint32_t *out, uint32_t capacity) {
    const uint32_t v[] = {(uint32_t)sizeof(f3d_session_paint_desc),
                          (uint32_t)offsetof(f3d_session_paint_desc, struct_size), (uint32_t)offsetof(f3d_session_paint_desc, flags),
                          (uint32_t)offsetof(f3d_session_paint_desc, primitive), (uint32_t)offsetof(f3d_session_paint_desc, vertex_count),
                          (uint32_t)offsetof(f3d_session_paint_desc, xz), (uint32_t)offsetof(f3d_session_paint_desc, rgba),
                          (uint32_t)offsetof(f3d_session_paint_desc, feature), (uint32_t)offsetof(f3d_session_paint_desc, indices),
                          (uint32_t)offsetof(f3d_session_paint_desc, index_count), (uint32_t)offsetof(f3d_session_paint_desc, half_width),
                          (uint32_t)offsetof(f3d_session_paint_desc, opacity), (uint32_t)offsetof(f3d_session_paint_desc, aim),
                          (uint32_t)sizeof(PaintPrim), kPaintTile, kPaintChunk};
    const uint32_t n = (uint32_t)(sizeof v / sizeof v[0]);
    for (uint32_t i = 0; i < n && i < capacity; i++) out[i] = v[i];
    return n;
}
