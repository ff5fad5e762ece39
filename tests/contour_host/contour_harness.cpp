// tests/contour_host/contour_harness.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_session_contour_host.py compiles it).
// The contour kernels' lane bodies (f3d_contour.h: what k_contour_count and k_contour_emit run per lane) on the host over whole
// 64-lane waves: wave b owns block b of the blocks the region touches, the count pass writes a total a block, a plain loop is
// the exclusive scan, the emit pass takes a lane's offset from the block's offset plus the exclusive prefix over the lanes --
// the reduction, the scan and the prefix written as loops, everything else the kernels' own code.
// With -DCONTOUR_DRIVER the file is a stand-alone program (its own main) over synthetic DEMs, for a sanitizer build.
#include "../emul/f3d_emul.cpp"
#include "../emul/host_scene.h"
#include "../../forge3d_amd/csrc/f3d_contour.h"

namespace {
// count, scan, emit.  cells / cases (capacity words each, may be null): the cell (cz * cell_w + cx) and the case of every record.
uint64_t run_contours(const TerrainDev &T, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, const float *levels, uint32_t level_count,
                      uint32_t cull, uint64_t capacity, float *segments, uint32_t *level_index, PaintPrim *prims, const float *rgba, uint32_t *cells,
                      uint32_t *cases) {
    ContourParams P{};
    P.terrain = T;
    P.row0 = row0, P.col0 = col0, P.rows = rows, P.cols = cols;
    contour_blocks(P);
    P.levels = levels;
    P.level_count = level_count;
    P.cull = cull;
    const uint32_t blocks = P.nbx * P.nbz;
    std::vector<uint64_t> totals((size_t)blocks + 1u, 0u), offsets((size_t)blocks + 1u, 0u);
    P.totals = totals.data();
    P.offsets = offsets.data();
    for (uint32_t b = 0; b < blocks; b++) {
        uint32_t sum = 0u;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            ContourLane L;
            if (contour_lane(P, b, lane, L)) sum += L.n;
        }
        totals[b] = sum;
    }
    for (uint32_t b = 0; b < blocks; b++) offsets[b + 1u] = offsets[b] + totals[b];
    P.capacity = capacity;
    P.segments = segments;
    P.level_index = level_index;
    P.prims = prims;
    if (rgba)
        for (int c = 0; c < 4; c++) P.rgba[c] = rgba[c];
    for (uint32_t b = 0; b < blocks; b++) {
        uint32_t prefix = 0u;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            ContourLane L;
            if (!contour_lane(P, b, lane, L)) break;
            const uint64_t at = offsets[b] + prefix;
            prefix += L.n;
            if (L.n == 0u) continue;
            contour_lane_emit(P, L.cx, L.cz, L.rec, L.l0, L.l1, at, [&](uint64_t i, float ax, float az, float bx, float bz, uint32_t k) {
                if (i >= P.capacity) return;
                if (P.prims) P.prims[i] = contour_prim(P.rgba, ax, az, bx, bz);
                if (P.segments) {
                    P.segments[4u * i] = ax, P.segments[4u * i + 1u] = az, P.segments[4u * i + 2u] = bx, P.segments[4u * i + 3u] = bz;
                }
                if (P.level_index) P.level_index[i] = k;
                if (cells) cells[i] = L.cz * T.cell_w + L.cx;
                if (cases) cases[i] = contour_case(L.rec, P.levels[k]);
            });
        }
    }
    return offsets[blocks];
}
}  // namespace

// info[0..3] = terrain origin x, origin z, spacing x, spacing z; dims[0..2] = cell_w, cell_h, mip_count
extern "C" void *contour_scene_create(const f3d_terrain_ref_desc *d, float *info, uint32_t *dims) {
    HostScene *S = new HostScene();
    try {
        setup(*S, d, 1, 0u, 0u);
    } catch (const Failure &) {
        delete S;
        return nullptr;
    }
    const TerrainDev &T = S->P.terrain;
    if (info) info[0] = T.origin_x, info[1] = T.origin_z, info[2] = T.spacing_x, info[3] = T.spacing_z;
    if (dims) dims[0] = T.cell_w, dims[1] = T.cell_h, dims[2] = T.mip_count;
    return S;
}

extern "C" void contour_scene_destroy(void *scene) { delete (HostScene *)scene; }

// the session's heights: sample (i, j) as the leaf table holds it
extern "C" void contour_heights(void *scene, float *out) {
    const TerrainDev &T = ((const HostScene *)scene)->P.terrain;
    for (uint32_t j = 0; j <= T.cell_h; j++)
        for (uint32_t i = 0; i <= T.cell_w; i++) {
            const uint32_t cx = i < T.cell_w ? i : T.cell_w - 1u, cz = j < T.cell_h ? j : T.cell_h - 1u;
            const LeafRec rec = T.leaves[tiled_index(cx, cz, T.tiles_x[0])];
            out[(size_t)j * (T.cell_w + 1u) + i] = pick4((i - cx) | ((j - cz) << 1), rec.h00, rec.h10, rec.h01, rec.h11);
        }
}

// One call as f3d_session_contours answers it (prims null) or as f3d_session_paint_contours fills the paint buffer (prims: 20
// words a record).  Returns the total.
extern "C" uint64_t contour_run(void *scene, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, const float *levels, uint32_t level_count,
                                uint32_t cull, uint64_t capacity, float *segments, uint32_t *level_index, void *prims, const float *rgba, uint32_t *cells,
                                uint32_t *cases) {
    return run_contours(((const HostScene *)scene)->P.terrain, row0, col0, rows, cols, levels, level_count, cull, capacity, segments, level_index,
                        (PaintPrim *)prims, rgba, cells, cases);
}

extern "C" uint32_t contour_desc_size(int paint) {
    return paint ? (uint32_t)sizeof(f3d_session_paint_contours_desc) : (uint32_t)sizeof(f3d_session_contours_desc);
}

#if defined(CONTOUR_DRIVER)
// A 65 x 63, a 10 x 9, a 5 x 3 and a 2 x 2 synthetic DEM; many levels (a sample's own height among them), one level, levels
// outside the range; whole and unaligned regions; with and without the cull; a capacity below the total; both output forms.
// Prints one line; exit status 0 when cull and no cull agree and every coordinate is finite.
int main() {
    unsigned long long segments_total = 0ull, bad = 0ull;
    double check = 0.0;
    const uint32_t shapes[4][2] = {{65u, 63u}, {10u, 9u}, {5u, 3u}, {2u, 2u}};
    for (const auto &shape : shapes) {
        const uint32_t w = shape[0], h = shape[1];
        std::vector<float> dem((size_t)w * h);
        for (uint32_t z = 0; z < h; z++)
            for (uint32_t x = 0; x < w; x++) dem[(size_t)z * w + x] = 3.0f * std::sin(0.37f * (float)x) * std::cos(0.23f * (float)z) + 0.05f * (float)((x * 7u + z * 13u) % 11u);
        HostTables t = build_tables_host(dem.data(), w, h, 20.0f);
        TerrainDev T{};
        t.attach(T);
        T.spacing_x = 30.0f;
        T.spacing_z = 25.0f;
        T.origin_x = -0.5f * ((float)w - 1.0f) * T.spacing_x;
        T.origin_z = -0.5f * ((float)h - 1.0f) * T.spacing_z;
        std::vector<float> many;
        for (int k = -700; k <= 700; k++) many.push_back(0.1f * (float)k);
        const float own = 20.0f * dem[dem.size() / 2u];
        std::vector<float> lists[4] = {many, {own}, {-1000.0f, -900.0f}, {900.0f, 1000.0f}};
        const float rgba[4] = {0.0f, 0.0f, 0.0f, 0.8f};
        for (const auto &levels : lists)
            for (int region = 0; region < 2; region++) {
                const uint32_t row0 = region && h > 3u ? 1u : 0u, col0 = region && w > 4u ? 2u : 0u;
                const uint32_t rows = region && h > 3u ? h - 3u : h - 1u, cols = region && w > 4u ? w - 4u : w - 1u;
                const uint64_t total = run_contours(T, row0, col0, rows, cols, levels.data(), (uint32_t)levels.size(), 1u, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
                std::vector<float> a((size_t)total * 4u + 4u, 77.0f), b((size_t)total * 4u + 4u, 77.0f);
                std::vector<uint32_t> ia((size_t)total + 1u), ib((size_t)total + 1u);
                std::vector<PaintPrim> prims((size_t)total / 2u + 1u);
                bad += run_contours(T, row0, col0, rows, cols, levels.data(), (uint32_t)levels.size(), 1u, total, a.data(), ia.data(), nullptr, nullptr, nullptr, nullptr) != total;
                bad += run_contours(T, row0, col0, rows, cols, levels.data(), (uint32_t)levels.size(), 0u, total, b.data(), ib.data(), nullptr, nullptr, nullptr, nullptr) != total;
                (void)run_contours(T, row0, col0, rows, cols, levels.data(), (uint32_t)levels.size(), 1u, total / 2u, nullptr, nullptr, prims.data(), rgba, nullptr, nullptr);
                for (size_t q = 0; q < (size_t)total * 4u; q++) {
                    bad += (a[q] != b[q] || !std::isfinite(a[q])) ? 1ull : 0ull;
                    check += a[q];
                }
                for (size_t q = 0; q < (size_t)total; q++) bad += ia[q] != ib[q] ? 1ull : 0ull;
                for (size_t q = 0; q < (size_t)(total / 2u); q++) bad += (prims[q].v[0] != a[4u * q] || prims[q].v[5] != a[4u * q + 3u]) ? 1ull : 0ull;
                bad += a[(size_t)total * 4u] != 77.0f ? 1ull : 0ull;
                segments_total += total;
            }
    }
    printf("contour driver: %llu segments, checksum %.9g, disagreements: %llu\n", segments_total, check, bad);
    return bad == 0ull ? 0 : 1;
}
#endif
