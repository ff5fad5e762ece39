// forge3d_amd/csrc/f3d_retable.hip -- the kernels of f3d_retable.h: a session's own leaf and band tables patched under a
// block of new DEM samples (f3d_session_reterrain).  Two launches whatever the DEM's size:
//   k_retable_tiles   one workgroup of 256 per aligned 64x64-cell tile the dirty range touches.  Level 0 of the tile goes
//                     into LDS (dirty cells: record patched and written; the others: their band as the table holds it;
//                     32 KB), then levels 1..6 are reduced there, 43.7 KB in all, a barrier between levels; only nodes of
//                     the dirty range are written to the band tables.
//   k_retable_top     ONE workgroup of 1024 walks the levels above (at most 64^2 + 32^2 + ... nodes for an 8192^2 DEM)
//                     through global memory: stores, fence, barrier, next level.
#include <hip/hip_runtime.h>

#include "f3d_retable.h"

namespace f3d {

namespace {

__global__ __launch_bounds__(256) void k_retable_tiles(const RetableParams P) {
    __shared__ NodeRec lds[kRetableTileRecords];
    const uint32_t tile = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < kRetableTile * kRetableTile; i += blockDim.x) retable_tile_level0(P, tile, lds, i);
    const uint32_t last = P.levels < kRetableTileLevels ? P.levels : kRetableTileLevels;
    for (uint32_t l = 1u; l < last; l++) {
        __syncthreads();
        const uint32_t n = kRetableTile >> l;
        for (uint32_t i = threadIdx.x; i < n * n; i += blockDim.x) retable_tile_level(P, tile, lds, l, i);
    }
}

__global__ __launch_bounds__(1024) void k_retable_top(const RetableParams P) {
    for (uint32_t l = kRetableTileLevels; l < P.levels; l++) {
        const uint32_t count = retable_top_count(P, l);
        for (uint32_t k = threadIdx.x; k < count; k += blockDim.x) retable_top_at(P, l, k);
        __threadfence();  // this level's records before anybody of the workgroup reads them for the next
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_retable(const RetableParams &P, hipStream_t stream) {
    hipLaunchKernelGGL(k_retable_tiles, dim3(P.tiles_x * P.tiles_y), dim3(256), 0, stream, P);
    hipLaunchKernelGGL(k_retable_top, dim3(1), dim3(1024), 0, stream, P);
    return hipGetLastError();
}

}  // namespace f3d
