// forge3d_amd/csrc/f3d_drainage.hip -- the kernels of f3d_drainage.h: D8 flow directions, flow accumulation, basins and the
// stream network of a session's terrain, routed on the device from the session's own leaf table.
//   k_drain_direction  one wave (a workgroup of 64) per 8 x 8 tile of samples aligned to the leaf table's tiles, lane l holds
//                      sample (l & 7, l >> 3) of it: the nine heights through lattice_height -- the wave's 64 stencils read its own
//                      tile's 1 KB run and a fringe of the neighbours' --, the code as a byte, round 0's pointer word (receiver |
//                      live bit), s = 1, depth 0; a ballot counts the wave's sinks, lane 0 adds them to the wave's slot of the
//                      call's counters
//   k_drain_jump       round k, one lane a sample in index order: q' = q[q], live' = live && live[q], s' = s (coalesced but
//                      for the one gather q[q]); a sample that stops being live learns its depth; the wave's live' lanes are
//                      counted into the wave's slot of the next round's counters, which the host reads back and sums to
//                      decide whether there is a next round
//   k_drain_add        round k: a live lane does one integer atomicAdd of s[v] into s'[q[v]]; its value is not used, so
//                      nothing waits for it; the order of arrival cannot change an integer sum
//   k_drain_write      the region's samples out of the final planes: direction, accumulation, basin
//   k_stream_count     one wave per 64 consecutive samples of the region, row-major: a ballot of "emits" is the wave's total
//   (the contours' scan: launch_contour_scan, 64-bit sums)
//   k_stream_emit      the same ballot again; a lane writes at its wave's offset plus the emitting lanes below it
// Nothing here keeps a value in LDS: the rounds are gathers and scatters over planes of w * h words.  Measured on the 2048^2
// proxy (profiles/README.md): k_drain_add leaves L2 as 64-byte atomic requests at 1.2 - 1.5 TB/s in the rounds with many live
// samples -- the chip-wide atomic rate, so it is atomic-bound there, and the requests grow from 0.65 M to 1.87 M as the
// receivers move 2^k samples away and stop sharing lines; k_drain_jump takes as long without an atomic, on its gather.
// The counters are slotted (f3d_drainage.h) because every wave adding into ONE word cost 0.7 ms a round.
#include <hip/hip_runtime.h>

#include "f3d_drainage.h"
#include "f3d_launch.h"

namespace f3d {

namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot, uint32_t lane) { return (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(64) void k_drain_direction(const DrainParams P) {
    const uint32_t lane = threadIdx.x;
    uint32_t i, j;
    const bool have = drain_tile_sample(P.w, P.h, blockIdx.x, lane, i, j);
    const bool sink = have && drain_lane_direction(P, i, j);
    const uint64_t sinks = __ballot(sink);
    if (lane == 0u && sinks != 0ull) atomicAdd(P.counters + kDrainSinks + (blockIdx.x & (kDrainSlots - 1u)), (uint32_t)__popcll(sinks));
}

__global__ __launch_bounds__(256) void k_drain_jump(const DrainParams P) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t depth = 0u;
    const bool next = v < P.w * P.h && drain_lane_jump(P, v, depth);
    const uint64_t live = __ballot(next);
    for (uint32_t m = 32u; m > 0u; m >>= 1) depth = max(depth, (uint32_t)__shfl_xor((int)depth, (int)m, 64));
    if (lane == 0u) {
        const uint32_t slot = (v >> 6) & (kDrainSlots - 1u);
        if (live != 0ull) atomicAdd(P.counters + kDrainLiveAt + (P.round + 1u) * kDrainSlots + slot, (uint32_t)__popcll(live));
        if (depth != 0u) atomicMax(P.counters + kDrainLongest + slot, depth);
    }
}

__global__ __launch_bounds__(256) void k_drain_add(const DrainParams P) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    uint32_t target, amount;
    if (v < P.w * P.h && drain_lane_add(P, v, target, amount)) atomicAdd(P.s_next + target, amount);
}

__global__ __launch_bounds__(256) void k_drain_write(const DrainParams P) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n < P.rows * P.cols) drain_lane_write(P, n);
}

__global__ __launch_bounds__(64) void k_stream_count(const DrainParams P) {
    const uint32_t wave = blockIdx.x, lane = threadIdx.x;
    uint32_t i, j, code, accumulation;
    // (the word behind the waves: the scan's last word is the total -- its wave has no sample and counts 0)
    const uint64_t emits = __ballot(stream_lane(P, wave * 64u + lane, i, j, code, accumulation));
    if (lane == 0u) P.totals[wave] = (uint64_t)__popcll(emits);
}

__global__ __launch_bounds__(64) void k_stream_emit(const DrainParams P) {
    const uint32_t wave = blockIdx.x, lane = threadIdx.x;
    uint32_t i, j, code, accumulation;
    const bool emit = stream_lane(P, wave * 64u + lane, i, j, code, accumulation);
    const uint64_t emits = __ballot(emit);
    if (!emit) return;
    const uint64_t at = P.offsets[wave] + lanes_below(emits, lane);
    if (at >= P.capacity) return;
    float ax, az, bx, bz;
    stream_segment(P.terrain, i, j, code, ax, az, bx, bz);
    if (P.prims) {
        contour_prim_store(P.prims + at, contour_prim(P.rgba, ax, az, bx, bz));
    } else {
        if (P.segments) *(float4 *)(P.segments + 4u * at) = float4{ax, az, bx, bz};
        if (P.stream_accumulation) P.stream_accumulation[at] = accumulation;
    }
}

hipError_t launched() { return hipGetLastError(); }

}  // namespace

hipError_t launch_drain_direction(const DrainParams &P, hipStream_t stream) {
    const hipError_t cleared = hipMemsetAsync(P.counters, 0, kDrainCounters * sizeof(uint32_t), stream);
    if (cleared != hipSuccess) return cleared;
    hipLaunchKernelGGL(k_drain_direction, dim3(drain_tiles(P.w, P.h)), dim3(64), 0, stream, P);
    return launched();
}

hipError_t launch_drain_round(const DrainParams &P, hipStream_t stream) {
    const uint32_t blocks = (P.w * P.h + 255u) / 256u;  // (w * h <= 2^31: no overflow)
    hipLaunchKernelGGL(k_drain_jump, dim3(blocks), dim3(256), 0, stream, P);
    hipError_t err = launched();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_drain_add, dim3(blocks), dim3(256), 0, stream, P);
    return launched();
}

hipError_t launch_drain_write(const DrainParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_drain_write, dim3((P.rows * P.cols + 255u) / 256u), dim3(256), 0, stream, P);
    return launched();
}

hipError_t launch_stream_count(const DrainParams &P, void *scan_tmp, size_t scan_bytes, hipStream_t stream) {
    const uint32_t waves = stream_waves(P.rows, P.cols);
    hipLaunchKernelGGL(k_stream_count, dim3(waves + 1u), dim3(64), 0, stream, P);
    const hipError_t err = launched();
    if (err != hipSuccess) return err;
    return launch_contour_scan(P.totals, (uint64_t *)P.offsets, waves, scan_tmp, scan_bytes, stream);
}

hipError_t launch_stream_emit(const DrainParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_stream_emit, dim3(stream_waves(P.rows, P.cols)), dim3(64), 0, stream, P);
    return launched();
}

}  // namespace f3d
