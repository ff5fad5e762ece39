// The layout arithmetic of the paint's, the contours', the drainage's and the fill's scratch (csrc/f3d_scratch_carve.h, which
// includes no HIP type) over a table of cases, the layouts put together as csrc/f3d_host_paint.h, f3d_host_contour.h and
// f3d_host_drainage.h put them together: a call's own pieces, then the host form's outputs carved behind them (what
// staged_carve of csrc/f3d_host_derived.h does with a list of outputs: an absent one takes 0 bytes).  argv[1]: the bytes of
// the scan's (and the sort's) storage, which on the device rocPRIM names.  One line a case:
//   family and its counts | offset of every piece, then of every output | total
// tests/test_scratch_carve_host.py compares them with the formulas each family carried when it laid its scratch out by hand.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../forge3d_amd/csrc/f3d_scratch_carve.h"

static const size_t kDrainCounterWords = 35u * 256u, kFillCounterWords = 4u * 256u;  // (f3d_drainage.h, f3d_fill.h)

// The outputs of a host-form call behind `base`: those of `subset` have their bytes, the others none.
static void outputs(std::vector<size_t> &at, size_t &total, size_t base, unsigned subset, std::initializer_list<size_t> bytes) {
    Carver c;
    unsigned k = 0u;
    for (size_t b : bytes) at.push_back(base + c.take((subset >> k++) & 1u ? b : 0u));
    total = base + c.at;
}

static void print(const char *head, const std::vector<size_t> &at, size_t total) {
    printf("%s |", head);
    for (size_t v : at) printf(" %zu", v);
    printf(" | %zu\n", total);
}

int main(int argc, char **argv) {
    const size_t scan = argc > 1 ? (size_t)strtoull(argv[1], nullptr, 10) : 0u;
    const size_t samples[] = {4u, 81u, 4096u, 4095u, 2049u * 2049u}, tile_counts[] = {1u, 2u, 4u}, groups[] = {1u, 2u, 65u}, level_counts[] = {1u, 64u, 65u},
                 records[] = {0u, 1u, 3u, 16u, 17u};
    char head[128];
    size_t total = 0u;
    for (size_t n : samples) {
        for (unsigned subset = 0u; subset < 8u; subset++) {
            // drainage: the routing's pieces, the three planes of the region (here the whole DEM) behind them
            Carver c;
            const DrainLayout D = drain_layout(c, n, kDrainCounterWords);
            std::vector<size_t> at = {D.counters, D.code, D.q, D.q_next, D.s, D.s_next, D.depth};
            outputs(at, total, c.at, subset, {n, 4u * n, 4u * n});
            snprintf(head, sizeof head, "drainage %zu %u", n, subset);
            print(head, at, total);
            for (size_t tiles : tile_counts) {
                // the fill alone, at offset 0 (f3d_session_fill) ...
                Carver alone;
                const FillLayout F = fill_layout(alone, n, tiles, kFillCounterWords);
                at = {F.counters, F.dirty[0], F.dirty[1], F.z, F.W, F.T};
                outputs(at, total, alone.at, subset, {4u * n, 4u * n, 4u * n});
                snprintf(head, sizeof head, "fill %zu %zu %u", n, tiles, subset);
                print(head, at, total);
                // ... and behind the routing's pieces (drain_route with F3D_DRAINAGE_FILL): the last column but one is its base
                Carver behind;
                const DrainLayout R = drain_layout(behind, n, kDrainCounterWords);
                const size_t fill_base = behind.at;
                const FillLayout G = fill_layout(behind, n, tiles, kFillCounterWords);
                at = {R.counters, R.code, R.q, R.q_next, R.s, R.s_next, R.depth, G.counters, G.dirty[0], G.dirty[1], G.z, G.W, G.T};
                outputs(at, total, behind.at, subset, {n, 4u * n, 4u * n});
                at.push_back(fill_base);
                snprintf(head, sizeof head, "filled-drainage %zu %zu %u", n, tiles, subset);
                print(head, at, total);
            }
        }
        // streams: the count layout without levels behind the routing's pieces (stream_count), then the records
        for (size_t waves : groups)
            for (size_t r : records)
                for (unsigned subset = 0u; subset < 4u; subset++) {
                    Carver routed;
                    drain_layout(routed, n, kDrainCounterWords);
                    Carver c;
                    const CountLayout L = count_layout(c, waves, 0u, scan);
                    std::vector<size_t> at = {routed.at + L.totals, routed.at + L.offsets, routed.at + L.scan};
                    outputs(at, total, routed.at + c.at, subset, {16u * r, 4u * r});
                    snprintf(head, sizeof head, "streams %zu %zu %zu %u", n, waves, r, subset);
                    print(head, at, total);
                }
    }
    for (size_t blocks : groups)
        for (size_t levels : level_counts)
            for (size_t r : records)
                for (unsigned subset = 0u; subset < 4u; subset++) {
                    Carver c;
                    const CountLayout L = count_layout(c, blocks, levels, scan);
                    std::vector<size_t> at = {L.totals, L.offsets, L.levels, L.scan};
                    outputs(at, total, c.at, subset, {16u * r, 4u * r});
                    snprintf(head, sizeof head, "contours %zu %zu %zu %u", blocks, levels, r, subset);
                    print(head, at, total);
                }
    for (size_t r : records) {
        Carver c;
        const PaintRecordsLayout L = paint_records_layout(c, r, 80u, scan);
        snprintf(head, sizeof head, "paint-records %zu", r);
        print(head, {L.records, L.counts, L.offsets, L.run_count, L.scan}, c.at);
        for (size_t tiles : tile_counts) {
            Carver k;
            const PaintKeysLayout K = paint_keys_layout(k, r, r < tiles ? r : tiles, scan);
            snprintf(head, sizeof head, "paint-keys %zu %zu", r, tiles);
            print(head, {K.keys, K.sorted, K.runs, K.sort}, k.at);
        }
    }
    return 0;
}
