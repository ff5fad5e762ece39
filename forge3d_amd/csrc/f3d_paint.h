// forge3d_amd/csrc/f3d_paint.h -- vector features painted onto the drape of a live session (f3d_session_paint): what one lane of
// k_paint does for its texel, and what one lane of the binning kernels does for its primitive.  Host and device: tests/paint_host
// runs both bodies on the CPU, and paint_texel() below -- every primitive of the call for one texel, no tiles -- is what the
// device must return, bit for bit.
//
// THE CONTRACT.  All arithmetic is f32, one rounding per written operation (the library and the host harness are compiled with
// -ffp-contract=off; nothing here spells an fma); division and sqrt are the correctly rounded forms.
//
// Geometry lives in world x-z.  Vertices are used exactly as given.  The centre of texel (r, c) of the drape is the inverse of
// drape_coords (f3d_drape.h),
//     x = origin_x + (((float)c - offset_x) / scale_x) * spacing_x          z = origin_z + (((float)r - offset_z) / scale_z) * spacing_z
// (scales may be negative), and  ramp = max(|spacing_x / scale_x|, |spacing_z / scale_z|)  is one texel in metres, computed once
// by the host.
//
// REACH.  A coordinate lies at most kPaintMaxReach = 2^16 texels from the terrain's centre: |x|, |z| <= 65536 ramp (the world's
// origin is the centre of the DEM; the largest canvas is 2^14 texels a side).  f3d_session_paint refuses a vertex beyond it.  The
// distance of a texel to a segment is formed from differences of coordinates, so its f32 error grows with them: a few 2^-23 of
// max(|p - a|, |b - a|) <= 2^17.5 ramp, below 0.1 ramp inside the reach -- and with it the error of a coverage, and of an edge
// function taken as a distance.  The slacks of the binning below (half a texel and more) are sized for that; beyond the reach a
// far vertex could give paint_texel a noisy coverage the tile lists do not bound.
//
// A call paints primitives of ONE kind, given as index lists; every primitive is a record of up to three vertices (x, z) with an
// RGBA colour each (paint_prim).
//   segment (a, b), half-width hw in metres, at p = the texel centre:
//       e = b - a,  q = p - a,  den = e.x e.x + e.z e.z
//       t = clamp((q.x e.x + q.z e.z) / den, 0, 1)          t = 0 when den == 0 (a == b)
//       d = sqrt(dx dx + dz dz),  dx = q.x - t e.x,  dz = q.z - t e.z
//       cov = clamp((hw - d) / ramp + 0.5, 0, 1)
//     round caps and joins follow from the distance; colour and alpha are  ca + t (cb - ca)  per channel.
//   point: the segment with a == b -- a disc.
//   triangle (v0, v1, v2): cov is 1 or 0, no edge ramp.  The edge function of an edge (p, q) at s is evaluated with the endpoints
//     in canonical order -- the lexicographically smaller (x, z) first -- and the sign flipped when they were swapped:
//       E(p, q; s) = (q.x - p.x) (s.z - p.z) - (q.z - p.z) (s.x - p.x)        (two products, one difference)
//     so two triangles that share an edge compute the same bits on it.  area = E(v0, v1; v2); a triangle with area == 0 paints
//     nothing; with o = sign(area):  w0 = o E(v1, v2; s), w1 = o E(v2, v0; s), w2 = o E(v0, v1; s).  The texel is inside when every
//     w_i > 0, or w_i == 0 and the edge owns its zeros (a top-left rule): with (dx, dz) = o (q - p) the edge's direction in the
//     triangle's positive winding, it owns them iff dz > 0 || (dz == 0 && dx < 0).  Colour and alpha are barycentric from the same
//     values: sum = (w0 + w1) + w2 (a texel with sum == 0 is outside), b1 = w1 / sum, b2 = w2 / sum,
//     c = (c0 + b1 (c1 - c0)) + b2 (c2 - c0)  -- exactly c0 for a triangle of one colour.
//
// Features.  Every primitive carries the number of its feature: the host numbers the runs of consecutive primitives whose
// first vertices have one feature id (without ids the whole call is run 0).  Per texel a feature's primitive is the one with the
// highest coverage, ties to the lowest index (a later primitive replaces the best only with cov > best), so polyline joints and
// overlapping triangles of one polygon do not blend twice under an opacity below 1.
//
// Blend.  Features blend in list order, in f32 registers:  a = (opacity * alpha) * cov,  dst = dst + a * (src - dst)  per channel;
// a feature with cov == 0 leaves the value bit-identical.  The texel is read with drape_texel's conversion and written once per
// call through drape_pack_texel; binary16 -> f32 -> binary16 is exact, so an untouched texel keeps its bits.
//
// THE RESULT NEVER DEPENDS ON TILING.  k_paint visits, per 16 x 16 tile of the canvas, the primitives the binning listed for the
// tile, in primitive order.  The lists are conservative (paint_bin: every texel with cov > 0 lies in a listed tile), a primitive
// with cov == 0 changes nothing of a lane's state (paint_visit), and a feature is flushed when the next visited primitive
// belongs to another run -- run numbers only rise --, so skipping primitives with cov == 0 returns paint_texel's bits.
//
// BINNING (paint_bin).  The primitive's bounding box in world x-z, grown by hw + ramp, is mapped through drape_coords' arithmetic
// to texel coordinates, padded by one texel on each side and clamped to the canvas: cov > 0 needs d < hw + ramp / 2, so the box
// has half a texel of the coarser axis plus a whole texel in hand against the roundings of the mapping (relative 2^-22 of a
// texel coordinate below 2^17) and of the distance (below 0.1 ramp inside the reach, at the texel and at the tile's centre).
// A stroke walks, per tile row of that range, only the columns of the part of the segment whose z lies within hw + ramp of the
// row's texel centres (the closest point of a covered texel lies there; that part's x extent, grown and padded like the box), so
// a long diagonal costs its length, not its box.  Its tiles are then tested against the capsule: the tile's texel centres lie in
// a disc of radius R (half the diagonal of the centres' extent) about the centre m of that extent, so a tile with
// dist(m, segment) > (hw + ramp + R) * (1 + 2^-13) holds no texel with cov > 0.  Triangles list their box.  The walk is the same
// in the count pass and in the emit pass.
#pragma once

#include "f3d_drape.h"

namespace f3d {

constexpr uint32_t kPaintPoints = 0u, kPaintLines = 1u, kPaintTriangles = 2u;
constexpr uint32_t kPaintTile = 16u;       // texels a side of a tile: one workgroup of 256 lanes
constexpr uint32_t kPaintChunk = 64u;      // primitive records staged through LDS at a time
constexpr uint32_t kPaintMaxPrims = 1u << 24;
constexpr float kPaintMaxReach = 65536.0f;  // texels from the terrain's centre a coordinate may lie (REACH above)
constexpr uint32_t kPaintPrimWords = 20u;

// One primitive: vertices a, b, c as (x, z) -- a segment uses a and b, a point a == b --, a colour per vertex, the feature run.
struct PaintPrim {
    float v[6];       // ax, az, bx, bz, cx, cz
    float c[12];      // RGBA of a, of b, of c
    uint32_t feature;
    uint32_t reserved;
};
static_assert(sizeof(PaintPrim) == kPaintPrimWords * sizeof(uint32_t), "k_paint stages a record as 20 words");

// The canvas: the session's drape (texels behind its 64-byte record), the DEM's frame and the drape's registration.
struct PaintCanvas {
    uint2 *texels;
    uint32_t rows, cols;
    float origin_x, origin_z, spacing_x, spacing_z;
    float scale_x, offset_x, scale_z, offset_z;
    float ramp;  // paint_ramp(): one texel in metres
};

struct PaintParams {
    PaintCanvas canvas;
    const PaintPrim *prims;
    uint32_t prim_count;
    uint32_t kind;          // kPaintPoints / kPaintLines / kPaintTriangles
    float half_width, opacity;
    // binning: counts[i] tiles of primitive i, offsets = their exclusive scan, keys = tile << 32 | primitive (sorted: per-tile
    // lists in primitive order), runs[k] = the first key of the k-th non-empty tile (any order), run_count their number
    // (counts and offsets hold prim_count + 1 words: offsets[prim_count] is the number of keys)
    uint64_t *counts;
    const uint64_t *offsets;
    uint64_t *keys;
    const uint64_t *sorted;
    uint32_t key_count;
    uint32_t *runs;
    uint32_t *run_count;
};

F3D_HD float paint_ramp(float spacing_x, float scale_x, float spacing_z, float scale_z) {
    return f_max(f_abs(spacing_x / scale_x), f_abs(spacing_z / scale_z));
}

F3D_HD void paint_centre(const PaintCanvas &C, uint32_t r, uint32_t c, float &x, float &z) {
    x = C.origin_x + (((float)c - C.offset_x) / C.scale_x) * C.spacing_x;
    z = C.origin_z + (((float)r - C.offset_z) / C.scale_z) * C.spacing_z;
}

// ---- coverage ---------------------------------------------------------------------------------------------------------------
// distance part of the segment rule: t and d of p = (x, z) against (a, b)
F3D_HD float paint_segment_distance(float ax, float az, float bx, float bz, float x, float z, float &t) {
    const float ex = bx - ax, ez = bz - az, qx = x - ax, qz = z - az;
    const float den = ex * ex + ez * ez;
    t = den == 0.0f ? 0.0f : f_clamp((qx * ex + qz * ez) / den, 0.0f, 1.0f);
    const float dx = qx - t * ex, dz = qz - t * ez;
    return f_sqrt(dx * dx + dz * dz);
}
F3D_HD float paint_segment_cov(const PaintPrim &p, float hw, float ramp, float x, float z, float &t) {
    const float d = paint_segment_distance(p.v[0], p.v[1], p.v[2], p.v[3], x, z, t);
    return f_clamp((hw - d) / ramp + 0.5f, 0.0f, 1.0f);
}

// E(p, q; s), endpoints in canonical order
F3D_HD float paint_edge(float px, float pz, float qx, float qz, float sx, float sz) {
    const bool swap = qx < px || (qx == px && qz < pz);
    const float ax = swap ? qx : px, az = swap ? qz : pz, bx = swap ? px : qx, bz = swap ? pz : qz;
    const float e = (bx - ax) * (sz - az) - (bz - az) * (sx - ax);
    return swap ? -e : e;
}
F3D_HD bool paint_edge_owns(float dx, float dz) { return dz > 0.0f || (dz == 0.0f && dx < 0.0f); }
F3D_HD bool paint_edge_in(float w, float dx, float dz) { return w > 0.0f || (w == 0.0f && paint_edge_owns(dx, dz)); }

// inside: b1, b2 the barycentric weights of v1 and v2
F3D_HD bool paint_triangle_in(const PaintPrim &p, float x, float z, float &b1, float &b2) {
    const float x0 = p.v[0], z0 = p.v[1], x1 = p.v[2], z1 = p.v[3], x2 = p.v[4], z2 = p.v[5];
    const float area = paint_edge(x0, z0, x1, z1, x2, z2);
    if (!(area != 0.0f) || area != area) return false;  // (zero, or NaN from an overflow)
    const float o = area > 0.0f ? 1.0f : -1.0f;
    const float w0 = o * paint_edge(x1, z1, x2, z2, x, z);
    const float w1 = o * paint_edge(x2, z2, x0, z0, x, z);
    const float w2 = o * paint_edge(x0, z0, x1, z1, x, z);
    const bool in = paint_edge_in(w0, o * (x2 - x1), o * (z2 - z1)) && paint_edge_in(w1, o * (x0 - x2), o * (z0 - z2)) &&
                    paint_edge_in(w2, o * (x1 - x0), o * (z1 - z0));
    const float sum = (w0 + w1) + w2;
    if (!in || !(sum > 0.0f)) return false;
    b1 = w1 / sum;
    b2 = w2 / sum;
    return true;
}

// ---- one lane: its texel's value, the feature being gathered ----------------------------------------------------------------------
struct PaintLane {
    float x, z;        // the texel centre
    V3 dst;
    uint32_t feature;  // the run whose best primitive is held
    float best;        // its coverage so far (0: none)
    float src[4];      // ... and its colour and alpha at this texel
};

F3D_HD void paint_begin(PaintLane &L, float x, float z, V3 dst) {
    L.x = x;
    L.z = z;
    L.dst = dst;
    L.feature = 0xFFFFFFFFu;
    L.best = 0.0f;
    L.src[0] = L.src[1] = L.src[2] = L.src[3] = 0.0f;
}
F3D_HD void paint_flush(PaintLane &L, float opacity) {
    if (L.best > 0.0f) {
        const float a = (opacity * L.src[3]) * L.best;
        L.dst.x = L.dst.x + a * (L.src[0] - L.dst.x);
        L.dst.y = L.dst.y + a * (L.src[1] - L.dst.y);
        L.dst.z = L.dst.z + a * (L.src[2] - L.dst.z);
    }
    L.best = 0.0f;
}
// the next primitive of the list (in primitive order; primitives with cov == 0 here may be left out)
F3D_HD void paint_visit(PaintLane &L, const PaintPrim &p, uint32_t kind, float hw, float ramp, float opacity) {
    if (p.feature != L.feature) {
        paint_flush(L, opacity);
        L.feature = p.feature;
    }
    if (kind == kPaintTriangles) {
        float b1, b2;
        if (!paint_triangle_in(p, L.x, L.z, b1, b2) || L.best >= 1.0f) return;
        L.best = 1.0f;
        for (uint32_t k = 0; k < 4u; k++) L.src[k] = (p.c[k] + b1 * (p.c[4u + k] - p.c[k])) + b2 * (p.c[8u + k] - p.c[k]);
    } else {
        float t;
        const float cov = paint_segment_cov(p, hw, ramp, L.x, L.z, t);
        if (!(cov > L.best)) return;
        L.best = cov;
        for (uint32_t k = 0; k < 4u; k++) L.src[k] = p.c[k] + t * (p.c[4u + k] - p.c[k]);
    }
}
F3D_HD V3 paint_end(PaintLane &L, float opacity) {
    paint_flush(L, opacity);
    return L.dst;
}

// Texel (r, c) after the call: every primitive, no tiles.  THE reference body: the device returns these bits.
// (paint_texel_value: the blended f32 value before it is rounded to binary16)
F3D_HD V3 paint_texel_value(const PaintParams &P, uint32_t r, uint32_t c) {
    const PaintCanvas &C = P.canvas;
    const uint2 t = C.texels[(size_t)r * C.cols + c];
    PaintLane L;
    float x, z;
    paint_centre(C, r, c, x, z);
    paint_begin(L, x, z, V3{drape_half(t.x & 0xFFFFu), drape_half(t.x >> 16), drape_half(t.y & 0xFFFFu)});
    for (uint32_t i = 0; i < P.prim_count; i++) paint_visit(L, P.prims[i], P.kind, P.half_width, C.ramp, P.opacity);
    return paint_end(L, P.opacity);
}
F3D_HD uint2 paint_texel(const PaintParams &P, uint32_t r, uint32_t c) {
    const V3 out = paint_texel_value(P, r, c);
    return drape_pack_texel(out.x, out.y, out.z);
}

// ---- binning ----------------------------------------------------------------------------------------------------------------
F3D_HD uint32_t paint_tiles_x(const PaintCanvas &C) { return (C.cols + kPaintTile - 1u) / kPaintTile; }
F3D_HD uint32_t paint_tiles_z(const PaintCanvas &C) { return (C.rows + kPaintTile - 1u) / kPaintTile; }

// texel indices [lo, hi] of an axis of n texels that texel coordinates between ta and tb, padded by a texel, can name
F3D_HD bool paint_axis_range(float ta, float tb, uint32_t n, uint32_t &lo, uint32_t &hi) {
    const float tmin = f_min(ta, tb) - 1.0f, tmax = f_max(ta, tb) + 1.0f;
    if (!(tmax >= 0.0f) || !(tmin <= (float)(n - 1u))) return false;
    lo = drape_clamp(f_floor(tmin), n);
    hi = drape_clamp(-f_floor(-tmax), n);
    return true;
}

// the tiles primitive p can touch, each given to f(tile) once, in rising order of tile = tile_z * tiles_x + tile_x
template <class F>
F3D_HD void paint_bin(const PaintCanvas &C, const PaintPrim &p, uint32_t kind, float hw, F &&f) {
    const bool tri = kind == kPaintTriangles;
    const float grow = hw + C.ramp;
    float x_lo = f_min(p.v[0], p.v[2]), x_hi = f_max(p.v[0], p.v[2]), z_lo = f_min(p.v[1], p.v[3]), z_hi = f_max(p.v[1], p.v[3]);
    if (tri) {
        x_lo = f_min(x_lo, p.v[4]), x_hi = f_max(x_hi, p.v[4]);
        z_lo = f_min(z_lo, p.v[5]), z_hi = f_max(z_hi, p.v[5]);
    }
    x_lo = x_lo - grow, x_hi = x_hi + grow, z_lo = z_lo - grow, z_hi = z_hi + grow;
    const float ta = ((x_lo - C.origin_x) / C.spacing_x) * C.scale_x + C.offset_x, tb = ((x_hi - C.origin_x) / C.spacing_x) * C.scale_x + C.offset_x;
    const float ua = ((z_lo - C.origin_z) / C.spacing_z) * C.scale_z + C.offset_z, ub = ((z_hi - C.origin_z) / C.spacing_z) * C.scale_z + C.offset_z;
    uint32_t c0, c1, r0, r1;
    if (!paint_axis_range(ta, tb, C.cols, c0, c1) || !paint_axis_range(ua, ub, C.rows, r0, r1)) return;
    const uint32_t tiles_x = paint_tiles_x(C);
    const float ax = p.v[0], az = p.v[1], ex = p.v[2] - p.v[0], ez = p.v[3] - p.v[1];
    for (uint32_t tz = r0 / kPaintTile; tz <= r1 / kPaintTile; tz++) {
        uint32_t t_lo = c0 / kPaintTile, t_hi = c1 / kPaintTile;
        if (!tri && ez != 0.0f) {
            // a stroke: only the part of the segment whose z lies within `grow` of the tile row's texel centres can reach them;
            // the columns are those of that part's x extent, grown and padded like the box (a long diagonal: a few tiles a row)
            const uint32_t re = tz * kPaintTile + (kPaintTile - 1u);
            float xa, za, xb, zb;
            paint_centre(C, tz * kPaintTile, 0u, xa, za);
            paint_centre(C, re < C.rows - 1u ? re : C.rows - 1u, 0u, xb, zb);
            const float s0 = ((f_min(za, zb) - grow) - az) / ez, s1 = ((f_max(za, zb) + grow) - az) / ez;
            const float u0 = f_max(f_min(s0, s1) - 0.0001220703125f, 0.0f), u1 = f_min(f_max(s0, s1) + 0.0001220703125f, 1.0f);
            if (u0 > u1) continue;  // (a NaN compares false: the row is walked)
            const float pa = ax + u0 * ex, pb = ax + u1 * ex;
            const float w_lo = f_min(pa, pb) - grow, w_hi = f_max(pa, pb) + grow;
            uint32_t k0, k1;
            if (!paint_axis_range(((w_lo - C.origin_x) / C.spacing_x) * C.scale_x + C.offset_x, ((w_hi - C.origin_x) / C.spacing_x) * C.scale_x + C.offset_x,
                                  C.cols, k0, k1))
                continue;
            t_lo = k0 / kPaintTile > t_lo ? k0 / kPaintTile : t_lo;
            t_hi = k1 / kPaintTile < t_hi ? k1 / kPaintTile : t_hi;
            if (t_lo > t_hi) continue;
        }
        for (uint32_t tx = t_lo; tx <= t_hi; tx++) {
            if (!tri) {
                // the tile's texel centres: a disc of radius R about m
                const uint32_t ce = tx * kPaintTile + (kPaintTile - 1u), re = tz * kPaintTile + (kPaintTile - 1u);
                float xa, za, xb, zb, t;
                paint_centre(C, tz * kPaintTile, tx * kPaintTile, xa, za);
                paint_centre(C, re < C.rows - 1u ? re : C.rows - 1u, ce < C.cols - 1u ? ce : C.cols - 1u, xb, zb);
                const float mx = 0.5f * (xa + xb), mz = 0.5f * (za + zb), rx = 0.5f * (xb - xa), rz = 0.5f * (zb - za);
                const float R = f_sqrt(rx * rx + rz * rz);
                const float d = paint_segment_distance(p.v[0], p.v[1], p.v[2], p.v[3], mx, mz, t);
                if (d > (grow + R) * 1.0001220703125f) continue;  // (a NaN distance lists the tile)
            }
            f(tz * tiles_x + tx);
        }
    }
}

}  // namespace f3d
