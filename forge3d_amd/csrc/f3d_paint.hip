// forge3d_amd/csrc/f3d_paint.hip -- the kernels of f3d_paint.h: vector features composited into a session's drape
// (f3d_session_paint).  Binning, then one workgroup per non-empty 16 x 16 tile of the canvas:
//   k_paint_count   one lane a primitive: the number of tiles it can touch (paint_bin)
//   (rocPRIM)       exclusive scan of the counts: where each primitive's keys go, and their total
//   k_paint_emit    one lane a primitive: its keys, tile << 32 | primitive, by the same walk
//   (rocPRIM)       radix sort of the keys: per-tile lists in primitive order, without an order-dependent atomic
//   k_paint_runs    one lane a key: the first key of every tile is appended to the run list (the order of the runs is free:
//                   tiles are independent of each other)
//   k_paint         one workgroup of 256 a run: lane (tid & 15, tid >> 4) holds its texel and the current feature's best
//                   coverage and colour in registers; the tile's primitive records pass through LDS 64 at a time (5 KB), every
//                   lane reading the same record (a broadcast: no bank conflict); a wave's four rows are whole 128-byte
//                   segments of 8-byte texels, read once and written once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "f3d_launch.h"
#include "f3d_paint.h"

namespace f3d {

namespace {

__global__ __launch_bounds__(256) void k_paint_count(const PaintParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > P.prim_count) return;
    uint64_t n = 0u;
    if (i < P.prim_count) paint_bin(P.canvas, P.prims[i], P.kind, P.half_width, [&](uint32_t) { n++; });
    P.counts[i] = n;  // (counts[prim_count] = 0: the scan's last word is the total)
}

__global__ __launch_bounds__(256) void k_paint_emit(const PaintParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.prim_count) return;
    uint64_t at = P.offsets[i];
    const uint64_t end = P.offsets[i + 1u];
    paint_bin(P.canvas, P.prims[i], P.kind, P.half_width, [&](uint32_t tile) {
        if (at < end) P.keys[at] = (uint64_t)tile << 32 | i;
        at++;
    });
}

__global__ __launch_bounds__(256) void k_paint_runs(const PaintParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.key_count) return;
    const uint32_t tile = (uint32_t)(P.sorted[i] >> 32);
    if (i == 0u || (uint32_t)(P.sorted[i - 1u] >> 32) != tile) P.runs[atomicAdd(P.run_count, 1u)] = i;
}

__global__ __launch_bounds__(256) void k_paint(const PaintParams P) {
    __shared__ uint32_t s_prim[kPaintChunk * kPaintPrimWords];
    __shared__ uint32_t s_ok[kPaintChunk];
    const PaintCanvas &C = P.canvas;
    const uint32_t tid = threadIdx.x;
    const uint32_t begin = P.runs[blockIdx.x];
    const uint32_t tile = (uint32_t)(P.sorted[begin] >> 32);
    const uint32_t tiles_x = paint_tiles_x(C);
    const uint32_t c = (tile % tiles_x) * kPaintTile + (tid & (kPaintTile - 1u)), r = (tile / tiles_x) * kPaintTile + tid / kPaintTile;
    const bool live = r < C.rows && c < C.cols;
    uint2 *texel = C.texels + ((size_t)r * C.cols + c);
    uint2 t = uint2{0u, 0u};
    if (live) t = *texel;
    PaintLane L;
    float x, z;
    paint_centre(C, r, c, x, z);
    paint_begin(L, x, z, V3{drape_half(t.x & 0xFFFFu), drape_half(t.x >> 16), drape_half(t.y & 0xFFFFu)});
    const uint32_t rec = tid >> 2, part = (tid & 3u) * (kPaintPrimWords / 4u);
    for (uint32_t base = begin;; base += kPaintChunk) {
        // four lanes a record, five words each; a record behind the tile's last key is marked absent
        const uint32_t at = base + rec;
        bool ok = false;
        if (at < P.key_count) {
            const uint64_t key = P.sorted[at];
            ok = (uint32_t)(key >> 32) == tile;
            if (ok) {
                const uint32_t *src = (const uint32_t *)(P.prims + (uint32_t)key) + part;
                for (uint32_t k = 0; k < kPaintPrimWords / 4u; k++) s_prim[rec * kPaintPrimWords + part + k] = src[k];
            }
        }
        if ((tid & 3u) == 0u) s_ok[rec] = ok ? 1u : 0u;
        __syncthreads();
        if (live)
            for (uint32_t j = 0; j < kPaintChunk && s_ok[j] != 0u; j++)
                paint_visit(L, *(const PaintPrim *)&s_prim[j * kPaintPrimWords], P.kind, P.half_width, C.ramp, P.opacity);
        const bool more = s_ok[kPaintChunk - 1u] != 0u;
        __syncthreads();
        if (!more) break;
    }
    if (live) {
        const V3 out = paint_end(L, P.opacity);
        *texel = drape_pack_texel(out.x, out.y, out.z);
    }
}

uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

uint32_t key_bits(uint32_t tiles) {  // of tile << 32 | primitive
    uint32_t bits = 1u;
    while (bits < 32u && (1u << bits) < tiles) bits++;
    return 32u + bits;
}

}  // namespace

hipError_t paint_scan_bytes(uint32_t prim_count, size_t *bytes) {
    *bytes = 0u;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0u, (size_t)prim_count + 1u,
                                   rocprim::plus<uint64_t>(), nullptr);
}

hipError_t paint_sort_bytes(uint32_t key_count, uint32_t tiles, size_t *bytes) {
    *bytes = 0u;
    return rocprim::radix_sort_keys(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, key_count, 0u, key_bits(tiles), nullptr);
}

hipError_t launch_paint_count(const PaintParams &P, void *scan_tmp, size_t scan_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(k_paint_count, dim3(blocks_of(P.prim_count + 1u)), dim3(256), 0, stream, P);
    return rocprim::exclusive_scan(scan_tmp, scan_bytes, (const uint64_t *)P.counts, (uint64_t *)P.offsets, (uint64_t)0u, (size_t)P.prim_count + 1u,
                                   rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_paint_bin(const PaintParams &P, uint32_t tiles, void *sort_tmp, size_t sort_bytes, hipStream_t stream) {
    hipError_t err = hipMemsetAsync(P.run_count, 0, sizeof(uint32_t), stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_paint_emit, dim3(blocks_of(P.prim_count)), dim3(256), 0, stream, P);
    err = rocprim::radix_sort_keys(sort_tmp, sort_bytes, (const uint64_t *)P.keys, (uint64_t *)P.sorted, P.key_count, 0u, key_bits(tiles), stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_paint_runs, dim3(blocks_of(P.key_count)), dim3(256), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_paint(const PaintParams &P, uint32_t run_count, hipStream_t stream) {
    hipLaunchKernelGGL(k_paint, dim3(run_count), dim3(256), 0, stream, P);
    return hipGetLastError();
}

}  // namespace f3d
