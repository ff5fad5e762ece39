// forge3d_amd/csrc/f3d_contour.hip -- the kernels of f3d_contour.h: contour lines of a session's terrain, extracted on the
// device (f3d_session_contours) or emitted straight into the paint rasteriser's primitive buffer (f3d_session_paint_contours).
// One wave (a workgroup of 64) per 8 x 8 block of cells the region touches:
//   k_contour_count  lane l holds cell (l >> 3, l & 7) of the block: its LeafRec through tiled_index -- the wave reads the
//                    block's 1 KB run once --, the block's level-3 band (a wave-uniform read) bisects the levels to those that
//                    can cross the block, a wave whose range is empty retires at once; each lane counts the segments of the
//                    levels inside its own cell's min and max; a wave reduction gives the block's total
//   (rocPRIM)        exclusive scan of the totals, 64-bit sums: where each block's records go, and their number
//   k_contour_emit   the same walk again; a lane writes at the block's offset plus the wave-exclusive prefix of its count
// The order of the output is therefore fixed without an atomic.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "f3d_contour.h"
#include "f3d_launch.h"

namespace f3d {

namespace {

__global__ __launch_bounds__(64) void k_contour_count(const ContourParams P) {
    const uint32_t block = blockIdx.x, lane = threadIdx.x;
    if (block >= P.nbx * P.nbz) {  // (the word behind the blocks: the scan's last word is the total)
        if (lane == 0u) P.totals[block] = 0u;
        return;
    }
    ContourLane L;
    uint32_t sum = 0u;
    if (contour_lane(P, block, lane, L)) {
        sum = L.n;  // (a lane holds at most 2 * kContourMaxLevels segments, a wave 2^23)
        for (uint32_t m = 32u; m > 0u; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)m, 64);
    }
    if (lane == 0u) P.totals[block] = sum;
}

__global__ __launch_bounds__(64) void k_contour_emit(const ContourParams P) {
    const uint32_t block = blockIdx.x, lane = threadIdx.x;
    ContourLane L;
    if (!contour_lane(P, block, lane, L)) return;
    uint32_t inclusive = L.n;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inclusive, d, 64);
        if (lane >= d) inclusive += up;
    }
    if (L.n == 0u) return;
    const uint64_t at = P.offsets[block] + (inclusive - L.n);
    if (P.prims) {
        contour_lane_emit(P, L.cx, L.cz, L.rec, L.l0, L.l1, at, [&](uint64_t i, float ax, float az, float bx, float bz, uint32_t) {
            if (i >= P.capacity) return;
            contour_prim_store(P.prims + i, contour_prim(P.rgba, ax, az, bx, bz));
        });
    } else {
        contour_lane_emit(P, L.cx, L.cz, L.rec, L.l0, L.l1, at, [&](uint64_t i, float ax, float az, float bx, float bz, uint32_t k) {
            if (i >= P.capacity) return;
            if (P.segments) *(float4 *)(P.segments + 4u * i) = float4{ax, az, bx, bz};
            if (P.level_index) P.level_index[i] = k;
        });
    }
}

}  // namespace

hipError_t contour_scan_bytes(uint32_t blocks, size_t *bytes) {
    *bytes = 0u;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0u, (size_t)blocks + 1u,
                                   rocprim::plus<uint64_t>(), nullptr);
}

hipError_t launch_contour_scan(const uint64_t *totals, uint64_t *offsets, uint32_t blocks, void *scan_tmp, size_t scan_bytes, hipStream_t stream) {
    return rocprim::exclusive_scan(scan_tmp, scan_bytes, totals, offsets, (uint64_t)0u, (size_t)blocks + 1u, rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_contour_count(const ContourParams &P, void *scan_tmp, size_t scan_bytes, hipStream_t stream) {
    const uint32_t blocks = P.nbx * P.nbz;
    hipLaunchKernelGGL(k_contour_count, dim3(blocks + 1u), dim3(64), 0, stream, P);
    const hipError_t launched = hipGetLastError();
    if (launched != hipSuccess) return launched;
    return launch_contour_scan(P.totals, (uint64_t *)P.offsets, blocks, scan_tmp, scan_bytes, stream);
}

hipError_t launch_contour_emit(const ContourParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_contour_emit, dim3(P.nbx * P.nbz), dim3(64), 0, stream, P);
    return hipGetLastError();
}

}  // namespace f3d
