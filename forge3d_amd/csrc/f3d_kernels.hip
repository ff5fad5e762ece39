// forge3d_amd/csrc/f3d_kernels.hip -- gfx950 kernels of the terrain path tracer.
// Host-callable launchers; the kernels themselves are in f3d_frame.h.
#include <type_traits>

#include "f3d_frame.h"

namespace f3d {

// ---- launchers ---------------------------------------------------------------------
void horizon_table_dims(uint32_t cell_w, uint32_t cell_h, uint32_t *level, uint32_t *bx, uint32_t *bz) {
    *level = horizon_block_level(cell_w, cell_h);
    *bx = (cell_w + (1u << *level) - 1u) >> *level;
    *bz = (cell_h + (1u << *level) - 1u) >> *level;
}
hipError_t launch_horizon_build(const TerrainDev &terrain, float *table, hipStream_t stream) {
    HorizonBuildParams B{};
    B.terrain = terrain;
    B.terrain.horizon = nullptr;
    horizon_table_dims(terrain.cell_w, terrain.cell_h, &B.level, &B.bx, &B.bz);
    B.table = table;
    hipLaunchKernelGGL(k_horizon_build, dim3(((B.bx + 7u) >> 3) * ((B.bz + 7u) >> 3)), dim3(kWave), 0, stream, B);
    return hipGetLastError();
}
// Workgroups of a launch over the band of p, one wave of `lanes` sample lanes a tile (f3d_tiles.h); the kernels that give
// every lane a pixel of its own (k_head, k_merge, k_gbuffer, ...) tile 8 x 8 whatever p.sample_lanes says: lanes = 1.
static inline TileGrid band_tiles(const FrameParams &p, uint32_t lanes) {
    return tile_grid(p.cam.width, p.band_end - p.band_begin, tile_shape(lanes));
}
static inline uint32_t frame_grid(const FrameParams &p, uint32_t lanes = 1u) { return launch_size(band_tiles(p, lanes), p.tile_map); }

// The instantiation table: a session's run-time sample-lane count and mesh flag as compile-time constants of a generic
// lambda, which names its kernel family once.  with_lanes: false = no kernel has that many sample lanes.
template <class F>
static bool with_lanes(uint32_t lanes, F &&launch) {
    switch (lanes) {
        case 1: launch(std::integral_constant<uint32_t, 1u>{}); return true;
        case 2: launch(std::integral_constant<uint32_t, 2u>{}); return true;
        case 4: launch(std::integral_constant<uint32_t, 4u>{}); return true;
        case 8: launch(std::integral_constant<uint32_t, 8u>{}); return true;
        default: return false;
    }
}
template <class F>
static void with_mesh(bool mesh, F &&launch) {
    if (mesh) launch(std::true_type{});
    else launch(std::false_type{});
}
static inline bool has_mesh(const FrameParams &p) { return p.mesh.traversal_mode == 0u; }

hipError_t launch_head(const FrameParams &p, hipStream_t stream) {  // the band's pixels, one lane each (8x8 tiles)
    if (frame_grid(p) == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_head, dim3(frame_grid(p)), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}

// Waves per SIMD the draped frame kernels are compiled for -- their own register budget ("Draping an image"):
// the sampled albedo makes the sun term and the IBL term per-lane values that live across the sun march (the undraped kernel
// forms them again from render constants).  At 80 VGPRs / 6 waves that costs scratch the undraped kernel does not have (terrain
// only: 12 against 8 B with 2, 4, 8 sample lanes, 76 against 44 B with one); at 96 VGPRs / 5 waves the 2-, 4- and 8-lane forms
// have none and the one-lane forms 36 B (terrain only) and 28 B (mesh), below the undraped kernel's 44 and 84.
#if !defined(F3D_DRAPE_WAVES)  // (6: A/B build, tools/build_variant.sh)
#define F3D_DRAPE_WAVES 5
#endif
constexpr int kDrapeWaves = F3D_DRAPE_WAVES;
hipError_t launch_frame(const FrameParams &p, int variant, hipStream_t stream) {
    const uint32_t lanes = sample_lanes_of(p);
    if (frame_grid(p, lanes) == 0u) return hipSuccess;  // an empty band
    const dim3 grid(frame_grid(p, lanes)), block(kWave);
    // (F3D_FORCE_MESH_KERNEL=1: A/B switch, the mesh-capable instantiation for a terrain-only scene -- same results)
    static const bool force_mesh = getenv("F3D_FORCE_MESH_KERNEL") != nullptr;
    const bool mesh = has_mesh(p) || force_mesh;
    const int budget = variant % 1000;  // 0: 80 VGPRs, 6 waves/SIMD; 104, 105: register-budget A/B variants
    bool known = false;
    if (p.drape) {  // a draped session: the default variant of each sample-lane count (the host refuses the A/B variants)
        known = budget == 0 && with_lanes(lanes, [&](auto S) {
            with_mesh(mesh, [&](auto M) { hipLaunchKernelGGL((k_frame_drape<kDrapeWaves, S(), M()>), grid, block, 0, stream, p); });
        });
    } else if (budget == 0) {  // one wave per workgroup
        known = with_lanes(lanes, [&](auto S) {
            with_mesh(mesh, [&](auto M) { hipLaunchKernelGGL((k_frame<0, 6, S(), M()>), grid, block, 0, stream, p); });
        });
    } else if (budget == 104 && lanes == 1u) {
        known = true;
        with_mesh(mesh, [&](auto M) { hipLaunchKernelGGL((k_frame<0, 4, 1u, M()>), grid, block, 0, stream, p); });
    } else if (budget == 105 && lanes == 4u) {
        known = true;
        with_mesh(mesh, [&](auto M) { hipLaunchKernelGGL((k_frame<0, 5, 4u, M()>), grid, block, 0, stream, p); });
    }
    return known ? hipGetLastError() : hipErrorInvalidValue;
}
// frames [p.frame_index, p.frame_index + frames) of the strip into p.trace (grid.y = frame)
hipError_t launch_trace(const FrameParams &p, uint32_t frames, hipStream_t stream) {
    const uint32_t lanes = sample_lanes_of(p);
    if (frame_grid(p, lanes) == 0u || frames == 0u) return hipSuccess;
    const dim3 grid(frame_grid(p, lanes), frames), block(kWave);
    const bool known = with_lanes(lanes, [&](auto S) {
        with_mesh(has_mesh(p), [&](auto M) { hipLaunchKernelGGL((k_trace<6, S(), M()>), grid, block, 0, stream, p); });
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}
// the wavefront form of launch_trace: primaries + queues, then the three queues through persistent waves
template <class K>
static uint32_t persistent_grid(K kernel) {
    int device = 0, cus = 256, per_cu = 0;
    (void)hipGetDevice(&device);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWave, 0) != hipSuccess || per_cu <= 0) per_cu = 16;
    return (uint32_t)cus * (uint32_t)per_cu;
}
hipError_t launch_trace_wavefront(const FrameParams &p, uint32_t frames, uint32_t quorum, hipStream_t stream) {
    const uint32_t lanes = sample_lanes_of(p);
    if (frame_grid(p, lanes) == 0u || frames == 0u) return hipSuccess;
    hipError_t err = hipMemsetAsync(p.wf.cursors, 0, 4u * sizeof(uint32_t), stream);
    if (err != hipSuccess) return err;
    const dim3 grid(frame_grid(p, lanes), frames), block(kWave);
    if (!with_lanes(lanes, [&](auto S) { hipLaunchKernelGGL((k_wf_primary<6, S()>), grid, block, 0, stream, p); }))
        return hipErrorInvalidValue;
    static const uint32_t sun_grid = persistent_grid(k_wf_occl<true, 7>), ibl_grid = persistent_grid(k_wf_occl<false, 8>);
    WfOcclParams W{};
    W.terrain = p.terrain;
    W.trace = p.trace;
    W.counts = p.wf.counts;
    W.regions = frames * p.wf.regions_per_frame;
    W.quorum = quorum;
    for (uint32_t q = 0u; q < 2u; q++) {  // sun rays along light.wi (front of the regions), along light.wi_reuse (back)
        if (q == 1u && p.same_sun != 0u) break;  // (the same bits: k_wf_primary files every sun ray at the front then)
        W.ray_o = p.wf.sun_o;
        W.ray_d = nullptr;
        W.ray_stop = p.wf.sun_stop;
        W.cursor = p.wf.cursors + q;
        W.kind = q;
        W.dir = q ? p.light.wi_reuse : p.light.wi;
        hipLaunchKernelGGL((k_wf_occl<true, 7>), dim3(sun_grid), block, 0, stream, W);
    }
    W.ray_o = p.wf.ibl_o;
    W.ray_d = p.wf.ibl_d;
    W.ray_stop = nullptr;
    W.cursor = p.wf.cursors + 2u;
    W.kind = 2u;
    hipLaunchKernelGGL((k_wf_occl<false, 8>), dim3(ibl_grid), block, 0, stream, W);
    return hipGetLastError();
}
hipError_t launch_trace_init(const FrameParams &p, hipStream_t stream) {
    if (frame_grid(p) == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_trace_init, dim3(frame_grid(p)), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_merge(const FrameParams &p, hipStream_t stream) {
    if (frame_grid(p) == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_merge, dim3(frame_grid(p)), dim3(kWave), 0, stream, p);  // (re-traces its mispredicted pixel-frames itself)
    return hipGetLastError();
}
hipError_t launch_tile_order(const FrameParams &p, const uint32_t *cost, uint32_t *order, hipStream_t stream) {
    const TileGrid tiles = band_tiles(p, sample_lanes_of(p));
    TileOrderParams B{cost, order, tiles.tiles_x, tiles.tiles_y};
    hipLaunchKernelGGL(k_tile_order, dim3(kNumXcd), dim3(1024), 0, stream, B);
    return hipGetLastError();
}
uint32_t frame_tile_count(const FrameParams &p, uint32_t *grid) {
    const uint32_t lanes = sample_lanes_of(p);
    if (grid) *grid = frame_grid(p, lanes);
    return band_tiles(p, lanes).count();
}
hipError_t launch_gbuffer(const FrameParams &p, float4 *gbuffer_n, float *depth, hipStream_t stream) {
    hipLaunchKernelGGL(k_gbuffer, dim3(frame_grid(p)), dim3(kWave), 0, stream, p, gbuffer_n, depth);
    return hipGetLastError();
}
static inline SkyBlockGeom sky_geom(const FrameParams &p) { return SkyBlockGeom{p.cam.width, p.cam.height, p.row_begin, p.row_end}; }
uint32_t sky_block_count(const FrameParams &p) { return sky_block_grid(sky_geom(p)).count(); }
hipError_t launch_sky_blocks(const FrameParams &p, uint32_t *blocks, bool enabled, hipStream_t stream) {
    const uint32_t count = sky_block_count(p);
    if (count == 0u || !blocks) return hipSuccess;
    const SkyBlocksParams B{p.primary_start, blocks, sky_geom(p), enabled ? 1u : 0u};
    hipLaunchKernelGGL(k_sky_blocks, dim3(count), dim3(kWave), 0, stream, B);
    return hipGetLastError();
}
hipError_t launch_rearm(const RearmParams &p, hipStream_t stream) {
    if (frame_grid(p.frame) == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_rearm, dim3(frame_grid(p.frame)), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_reaim(const RearmParams &p, hipStream_t stream) {
    if (frame_grid(p.frame) == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_reaim, dim3(frame_grid(p.frame)), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_resolve(const ResolveParams &p, hipStream_t stream) {
    if (p.frame.drape) hipLaunchKernelGGL(k_resolve_drape, dim3(frame_grid(p.frame)), dim3(kWave), 0, stream, p);
    else hipLaunchKernelGGL(k_resolve, dim3(frame_grid(p.frame)), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_drape_pack(const DrapePackParams &p, hipStream_t stream) {
    if (p.rows == 0u || p.cols == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_drape_pack, dim3((p.cols + 255u) / 256u, p.rows), dim3(256), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_ray_batch(const RayBatchParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(k_ray_batch, dim3((p.n + kWave - 1) / kWave), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_query(const QueryParams &p, hipStream_t stream) {
    if (p.count == 0u) return hipSuccess;
    const dim3 grid((p.count + kWave - 1u) / kWave), block(kWave);
    with_mesh(has_mesh(p.frame), [&](auto M) { hipLaunchKernelGGL((k_query<M()>), grid, block, 0, stream, p); });
    return hipGetLastError();
}
hipError_t launch_raster(const RasterParams &p, hipStream_t stream) {
    const uint32_t total = p.rows * p.cols;
    if (total == 0u || p.target_count == 0u) return hipSuccess;
    const dim3 grid((total + kWave - 1u) / kWave), block(kWave);
    with_mesh(has_mesh(p.frame), [&](auto M) { hipLaunchKernelGGL((k_raster<M()>), grid, block, 0, stream, p); });
    return hipGetLastError();
}
// k_horizon, k_clearance, k_umbra: one wave a workgroup over the region's waves; `count` planes, none: nothing to do
template <class Params>
static hipError_t launch_region(void (*kernel)(Params), const Params &p, uint32_t count, hipStream_t stream) {
    if (p.rows * p.cols == 0u || count == 0u) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(region_waves(p.rows, p.cols, p.block)), dim3(kWave), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_horizon(const HorizonParams &p, hipStream_t stream) { return launch_region(k_horizon, p, p.azimuth_count, stream); }
hipError_t launch_clearance(const ClearanceParams &p, hipStream_t stream) { return launch_region(k_clearance, p, p.observer_count, stream); }
hipError_t launch_umbra(const UmbraParams &p, hipStream_t stream) { return launch_region(k_umbra, p, p.direction_count, stream); }
hipError_t launch_irradiation(const IrradiationParams &p, hipStream_t stream) {
    const uint32_t total = p.rows * p.cols;
    if (total == 0u) return hipSuccess;
    const dim3 grid((total + kWave - 1u) / kWave), block(kWave);
    with_mesh(has_mesh(p.frame), [&](auto M) { hipLaunchKernelGGL((k_irradiation<M()>), grid, block, 0, stream, p); });
    return hipGetLastError();
}
hipError_t launch_leaf_build(const PyramidBuildParams &p, hipStream_t stream) {
    dim3 block(16, 16), grid((p.leaf_dim_x + 15) / 16, (p.leaf_dim_y + 15) / 16);
    hipLaunchKernelGGL(k_leaf_build, grid, block, 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_band_build(const BandBuildParams &p, hipStream_t stream) {
    dim3 block(16, 16), grid((p.width + 15) / 16, (p.height + 15) / 16);
    hipLaunchKernelGGL(k_band_build, grid, block, 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_level_build(const LevelBuildParams &p, hipStream_t stream) {
    dim3 block(16, 16), grid((p.dst_dim_x + 15) / 16, (p.dst_dim_y + 15) / 16);
    hipLaunchKernelGGL(k_level_build, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace f3d

#if defined(F3D_MESH_STATS)  // diagnostics build only (tools/experiments/c4_window.py): not part of the ABI
extern "C" int f3d_debug_mesh_stats(unsigned long long *out, int reset) {
    if (reset) {
        unsigned long long zero[8] = {};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(f3d::g_mesh_stats), zero, sizeof(zero));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(f3d::g_mesh_stats), 8 * sizeof(unsigned long long));
}
#endif
