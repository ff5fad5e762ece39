// forge3d_amd/csrc/f3d_fill.hip -- the kernels of f3d_fill.h: the filled surface of a session's terrain, the distance across
// its flats, and the D8 direction pass over both that k_drain_jump / k_drain_add continue from.
//   k_fill_init       one lane a sample in index order: z out of the leaf table into a plane of its own (4 bytes a sample, so
//                     that a round stages words, not 16-byte records), W0 = z on outlets and +inf elsewhere; the first
//                     fill_tiles() lanes mark every tile dirty
//   k_fill_relax      one workgroup of 4 * kFillTile threads per tile of kFillTile^2 samples.  A tile that is not dirty leaves
//                     after reading its flag.  Otherwise: the z and W planes of the tile with a one-sample halo into LDS
//                     (2 x 66 x 67 words = 35 KB of the CU's 160 KiB: four tiles a CU), then sweeps -- wave d walks the tile's
//                     64 lines in direction d, a lane a line, sample by sample -- until a sweep lowers nothing; one barrier a
//                     sweep and three rotating "changed" words (sweep n sets word n % 3, reads it behind the barrier, and
//                     thread 0 clears word (n + 2) % 3, which nobody reads or sets before the next barrier).  The changed
//                     samples go back to the W plane; the neighbour tiles that stage one of them are marked dirty for the next
//                     round, and every newly marked tile is counted into the round's slotted counter set.
//                     WHY RACING READS ARE RIGHT (f3d_fill.h): a lane of a sweep, and a halo load of another workgroup of
//                     the same round, may read a word before or after its owner lowered it.  Both values are upper bounds of
//                     the fixed point and the update only selects among what it read, so a stale read can delay a sample, not
//                     spoil it: inside a tile the sweep that lowered something is followed by another, across tiles a lowered
//                     edge sample marks every tile that staged it.  Words are 32-bit and aligned: no read sees half a value.
//   k_flat_init       one lane a sample: T0 = 0 on outlets and on samples with a strictly lower neighbour in W, else
//                     0xFFFFFFFF; only tiles that hold an undrained sample start dirty (and are counted)
//   k_flat_relax      k_fill_relax's shape over (W, T)
//   k_fill_direction  k_drain_direction's shape, a wave per 8 x 8 tile: fill_direction from the W and T planes; the code byte,
//                     round 0's pointer word, s = 1, depth 0, the sinks counted
//   k_fill_stats      the samples with W > z and the largest T, ballots and wave maxima into slotted counters
//   k_fill_write      the region's samples: W, W - z, T
// Counters are vector atomics on slotted words, as the drainage's.
#include <hip/hip_runtime.h>

#include "f3d_fill.h"
#include "f3d_launch.h"

namespace f3d {

namespace {

__global__ __launch_bounds__(256) void k_fill_init(const FillParams P) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < P.w * P.h) fill_lane_init(P, v);
}

// a tile newly marked in `plane` counts once, into the marking workgroup's slot of `set`
__device__ __forceinline__ void mark_tile(const FillParams &P, uint32_t plane, uint32_t other, uint32_t slot) {
    if (atomicExch(P.dirty[plane] + other, 1u) == 0u) atomicAdd(P.counters + kFillMarks + plane * kDrainSlots + slot, 1u);
}

template <class Rule>
__global__ __launch_bounds__(4 * kFillTile) void k_relax(const FillParams P) {
    typedef FillTileBody<kFillTile, Rule> Body;
    __shared__ typename Rule::A a[Body::kWords];
    __shared__ typename Rule::B b[Body::kWords];
    __shared__ uint32_t changed[3], touched;
    const uint32_t tile = blockIdx.x, t = threadIdx.x, now = P.round & 1u, next = now ^ 1u;
    if (tile == 0u)
        for (uint32_t n = t; n < kDrainSlots; n += Body::kThreads) P.counters[kFillMarks + now * kDrainSlots + n] = 0u;
    if (P.dirty[now][tile] == 0u) return;  // (uniform: one word for the workgroup)
    __syncthreads();                       // (everybody has read the flag before thread 0 clears it)
    if (t == 0u) P.dirty[now][tile] = 0u, changed[0] = changed[1] = changed[2] = touched = 0u;
    Body::load(P, tile, t, a, b);
    __syncthreads();
    for (uint32_t n = 0u;; n = n == 2u ? 0u : n + 1u) {
        if (Body::sweep(t, a, b)) changed[n] = 1u;
        __syncthreads();
        if (t == 0u) changed[n >= 1u ? n - 1u : 2u] = 0u;  // (word (n + 2) % 3)
        if (changed[n] == 0u) break;
    }
    const uint32_t mine = Body::store(P, tile, t, b);
    if (mine != 0u) atomicOr(&touched, mine);
    __syncthreads();
    uint32_t other;
    if (t < 8u && ((touched >> t) & 1u) != 0u && Body::neighbour(P, tile, t, other)) mark_tile(P, next, other, tile & (kDrainSlots - 1u));
}

__global__ __launch_bounds__(256) void k_flat_init(const FillParams P) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < P.w * P.h && flat_lane_init(P, v)) {
        const uint32_t tile = fill_tile_of(P, v);
        if (P.dirty[0][tile] == 0u) mark_tile(P, 0u, tile, (v >> 6) & (kDrainSlots - 1u));
    }
}

__global__ __launch_bounds__(64) void k_fill_direction(const DrainParams P) {
    const uint32_t lane = threadIdx.x;
    uint32_t i, j;
    const bool have = drain_tile_sample(P.w, P.h, blockIdx.x, lane, i, j);
    const bool sink = have && fill_lane_direction(P, i, j);
    const uint64_t sinks = __ballot(sink);
    if (lane == 0u && sinks != 0ull) atomicAdd(P.counters + kDrainSinks + (blockIdx.x & (kDrainSlots - 1u)), (uint32_t)__popcll(sinks));
}

__global__ __launch_bounds__(256) void k_fill_stats(const FillParams P) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t flat = 0u;
    const bool filled = v < P.w * P.h && fill_lane_stats(P, v, flat);
    if (v >= P.w * P.h) flat = 0u;
    const uint64_t all = __ballot(filled);
    for (uint32_t m = 32u; m > 0u; m >>= 1) flat = max(flat, (uint32_t)__shfl_xor((int)flat, (int)m, 64));
    if (lane == 0u) {
        const uint32_t slot = (v >> 6) & (kDrainSlots - 1u);
        if (all != 0ull) atomicAdd(P.counters + kFillFilled + slot, (uint32_t)__popcll(all));
        if (flat != 0u) atomicMax(P.counters + kFillLargest + slot, flat);
    }
}

__global__ __launch_bounds__(256) void k_fill_write(const FillParams P) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n < P.rows * P.cols) fill_lane_write(P, n);
}

hipError_t launched() { return hipGetLastError(); }

uint32_t sample_blocks(const FillParams &P) { return (P.w * P.h + 255u) / 256u; }  // (w * h <= 2^31: no overflow)

}  // namespace

hipError_t launch_fill_init(const FillParams &P, hipStream_t stream) {
    const hipError_t cleared = hipMemsetAsync(P.counters, 0, kFillCounters * sizeof(uint32_t), stream);
    if (cleared != hipSuccess) return cleared;
    hipLaunchKernelGGL(k_fill_init, dim3(sample_blocks(P)), dim3(256), 0, stream, P);
    return launched();
}

hipError_t launch_fill_relax(const FillParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_relax<FillRule>, dim3(fill_tiles(P.w, P.h, kFillTile)), dim3(4u * kFillTile), 0, stream, P);
    return launched();
}

hipError_t launch_flat_init(const FillParams &P, hipStream_t stream) {
    // (nothing to clear: in the fill's last round every tile that ran cleared its own flag and marked nobody, its tile 0 cleared
    // the counter set of the round before, and the set the host then read summed to 0)
    hipLaunchKernelGGL(k_flat_init, dim3(sample_blocks(P)), dim3(256), 0, stream, P);
    return launched();
}

hipError_t launch_flat_relax(const FillParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_relax<FlatRule>, dim3(fill_tiles(P.w, P.h, kFillTile)), dim3(4u * kFillTile), 0, stream, P);
    return launched();
}

hipError_t launch_fill_direction(const DrainParams &P, hipStream_t stream) {
    const hipError_t cleared = hipMemsetAsync(P.counters, 0, kDrainCounters * sizeof(uint32_t), stream);
    if (cleared != hipSuccess) return cleared;
    hipLaunchKernelGGL(k_fill_direction, dim3(drain_tiles(P.w, P.h)), dim3(64), 0, stream, P);
    return launched();
}

hipError_t launch_fill_stats(const FillParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_fill_stats, dim3(sample_blocks(P)), dim3(256), 0, stream, P);
    return launched();
}

hipError_t launch_fill_write(const FillParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_fill_write, dim3((P.rows * P.cols + 255u) / 256u), dim3(256), 0, stream, P);
    return launched();
}

}  // namespace f3d
