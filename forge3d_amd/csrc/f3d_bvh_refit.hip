// forge3d_amd/csrc/f3d_bvh_refit.hip -- the kernels of f3d_bvh_refit.h: a session's mesh BVH refitted on the GPU after its
// vertices moved (f3d_session_remesh with the session's topology).  Three launches a refit, a fourth the first time:
//   k_remesh_gather   leaf-order triangles in a grid-stride loop; scene bounds by wave and block reduction, then ordered-int
//                     atomics as k_prims has them, one set a block
//   k_remesh_link     one thread per node / record: parent links (first refit only)
//   k_remesh_refit    one thread per node (binary form) or record (four-wide form): leaf boxes, then bottom-up with one
//                     arrival counter per node -- the scheme of f3d_lbvh.hip k_refit: stores, __threadfence, the atomic
//                     arrival; the last to arrive fences again and reads the children with agent-scope loads
// No host wait anywhere: the padding is computed on the device from the bounds the gather pass left.
#include <hip/hip_runtime.h>

#include "f3d_bvh_refit.h"

namespace f3d {

namespace {

struct RefitDevice {  // (host-and-device signatures for the shared bodies; only the kernels instantiate them)
    static F3D_HD uint32_t arrive(uint32_t *counter) {
#if defined(__HIP_DEVICE_COMPILE__)
        return atomicAdd(counter, 1u);
#else
        return (*counter)++;
#endif
    }
    static F3D_HD float load(const float *p) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
        return *p;
#endif
    }
    static F3D_HD void fence() {
#if defined(__HIP_DEVICE_COMPILE__)
        __threadfence();
#endif
    }
};

// (a grid-stride loop and one set of atomics a BLOCK: with one set a wave, as k_prims has them, the 56 000 atomics of a
// 600 000-triangle mesh on six addresses were the kernel's whole time, 0.65 ms; the traffic itself is 75 MB)
constexpr uint32_t kGatherBlocks = 1024u;

__global__ __launch_bounds__(256) void k_remesh_gather(const RefitParams P) {
    __shared__ float part[4][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (blockIdx.x == 0u && threadIdx.x == 0u) refit_bounds_reset(P.bounds_next);  // (nobody else touches the other set during this refit)
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < P.tri_count; k += gridDim.x * blockDim.x) {
        float l[3], h[3];
        refit_gather_tri(P, k, l, h);
        for (int a = 0; a < 3; a++) {
            lo[a] = f_min(lo[a], l[a]);
            hi[a] = f_max(hi[a], h[a]);
        }
    }
    for (int a = 0; a < 3; a++) {
        float l = lo[a], h = hi[a];
        for (int off = 32; off > 0; off >>= 1) {
            l = f_min(l, __shfl_xor(l, off, 64));
            h = f_max(h, __shfl_xor(h, off, 64));
        }
        if ((threadIdx.x & 63u) == 0u) {
            part[threadIdx.x >> 6][a] = l;
            part[threadIdx.x >> 6][3 + a] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const uint32_t a = threadIdx.x;
        atomicMin(&P.bounds[a], refit_ordered(f_min(f_min(part[0][a], part[1][a]), f_min(part[2][a], part[3][a]))));
        atomicMax(&P.bounds[3u + a], refit_ordered(f_max(f_max(part[0][3u + a], part[1][3u + a]), f_max(part[2][3u + a], part[3][3u + a]))));
    }
}

__global__ __launch_bounds__(256) void k_remesh_link(const RefitParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (P.wide) {
        if (i < P.wide_count) refit_link_wide(P, i);
    } else if (i < P.node_count) {
        refit_link_binary(P, i);
    }
}

__global__ __launch_bounds__(256) void k_remesh_refit_binary(const RefitParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.node_count) refit_binary_node<RefitDevice>(P, i);
}

__global__ __launch_bounds__(256) void k_remesh_refit_wide(const RefitParams P) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < P.wide_count) refit_wide_node<RefitDevice>(P, w);
}

}  // namespace

hipError_t launch_bvh_refit(const RefitParams &P, bool link, hipStream_t stream) {
    const uint32_t n = P.wide ? P.wide_count : P.node_count;
    if (P.tri_count == 0u || n == 0u) return hipSuccess;
    const dim3 block(256);
    const uint32_t gather_blocks = (P.tri_count + 255u) / 256u;
    hipLaunchKernelGGL(k_remesh_gather, dim3(gather_blocks < kGatherBlocks ? gather_blocks : kGatherBlocks), block, 0, stream, P);
    if (link) hipLaunchKernelGGL(k_remesh_link, dim3((n + 255u) / 256u), block, 0, stream, P);
    if (P.wide) hipLaunchKernelGGL(k_remesh_refit_wide, dim3((n + 255u) / 256u), block, 0, stream, P);
    else hipLaunchKernelGGL(k_remesh_refit_binary, dim3((n + 255u) / 256u), block, 0, stream, P);
    return hipGetLastError();
}

}  // namespace f3d
