// forge3d_amd/csrc/f3d_launch.h -- host-callable launchers of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "f3d_aether.h"
#include "f3d_build.h"
#include "f3d_drape.h"
#include "f3d_paint.h"
#include "f3d_scene.h"

namespace f3d {

struct RayBatchParams {
    TerrainDev terrain;
    const float4 *rays;  // 2 float4 per ray: (origin, tmin), (direction, tmax)
    uint32_t n;
    uint32_t any_hit, apply_curvature;  // any_hit: 0 closest / 1 any-hit (sorted descent), 2 any / 3 closest (march)
    uint32_t start_in_cell;             // march only: start in the origin cell instead of at the root
    uint32_t *out_hit;
    float *out_t;
    float *out_normal;  // 3 per ray
};

struct ResolveParams {
    FrameParams frame;  // res_in = final temporal output, frame_index unused
    uint32_t frames;
    uint8_t *rgba;
    float *albedo, *normal;
    AetherDev aether;    // enabled = 0: the plain Reinhard resolve
    const float *depth;  // frame-0 depth AOV (the aerial-perspective post's segment length)
};

hipError_t launch_head(const FrameParams &p, hipStream_t stream);  // sample-lane form: before launch_frame
hipError_t launch_frame(const FrameParams &p, int variant, hipStream_t stream);
hipError_t launch_trace(const FrameParams &p, uint32_t frames, hipStream_t stream);  // frames in flight: a batch of frames
hipError_t launch_trace_wavefront(const FrameParams &p, uint32_t frames, uint32_t quorum, hipStream_t stream);  // same records, rays through queues
hipError_t launch_merge(const FrameParams &p, hipStream_t stream);
hipError_t launch_trace_init(const FrameParams &p, hipStream_t stream);               // first sun-direction predictions                   // ... and the ordered half of one
// longest-first dispatch of the frame kernel: tile count (and grid) of the current band, and the ordering kernel
uint32_t frame_tile_count(const FrameParams &p, uint32_t *grid);
hipError_t launch_tile_order(const FrameParams &p, const uint32_t *cost, uint32_t *order, hipStream_t stream);
hipError_t launch_gbuffer(const FrameParams &p, float4 *gbuffer_n, float *depth, hipStream_t stream);
// the deep-sky table of the strip of p (f3d_skyblocks.h) from p.primary_start; enabled = false: every block "not deep"
hipError_t launch_sky_blocks(const FrameParams &p, uint32_t *blocks, bool enabled, hipStream_t stream);
uint32_t sky_block_count(const FrameParams &p);  // blocks of the strip of p
hipError_t launch_rearm(const RearmParams &p, hipStream_t stream);  // same grid and pixel mapping as launch_gbuffer
hipError_t launch_reaim(const RearmParams &p, hipStream_t stream);  // ... and its LDS: the G-buffer pass and the re-arm in one
hipError_t launch_resolve(const ResolveParams &p, hipStream_t stream);  // (a draped session: the draped resolve)
hipError_t launch_drape_pack(const DrapePackParams &p, hipStream_t stream);  // f32 texels into a session's binary16 drape (f3d_drape.h)
// vector features into a session's drape (f3d_paint.h, f3d_paint.hip): the temporary storage of the scan over prim_count + 1
// counts and of the key sort; count pass + scan (offsets[prim_count] = the number of keys); emit + sort + run list (P.keys,
// P.sorted: key_count words each, P.runs: min(key_count, tiles) words, P.run_count: one); k_paint over run_count tiles
hipError_t paint_scan_bytes(uint32_t prim_count, size_t *bytes);
hipError_t paint_sort_bytes(uint32_t key_count, uint32_t tiles, size_t *bytes);
hipError_t launch_paint_count(const PaintParams &p, void *scan_tmp, size_t scan_bytes, hipStream_t stream);
hipError_t launch_paint_bin(const PaintParams &p, uint32_t tiles, void *sort_tmp, size_t sort_bytes, hipStream_t stream);
hipError_t launch_paint(const PaintParams &p, uint32_t run_count, hipStream_t stream);
// contour lines of a session's terrain (f3d_contour.h, f3d_contour.hip): the temporary storage of the scan over blocks + 1
// totals; count pass + scan (P.totals, P.offsets: nbx * nbz + 1 words each, offsets[nbx * nbz] = the number of segments); the
// emit pass into P.segments / P.level_index or P.prims, the first P.capacity records
struct ContourParams;
hipError_t contour_scan_bytes(uint32_t blocks, size_t *bytes);
hipError_t launch_contour_count(const ContourParams &p, void *scan_tmp, size_t scan_bytes, hipStream_t stream);
hipError_t launch_contour_emit(const ContourParams &p, hipStream_t stream);
// ... and that scan on its own: the exclusive scan of blocks + 1 totals into offsets (the stream network's waves use it too)
hipError_t launch_contour_scan(const uint64_t *totals, uint64_t *offsets, uint32_t blocks, void *scan_tmp, size_t scan_bytes, hipStream_t stream);
// drainage of a session's terrain (f3d_drainage.h, f3d_drainage.hip): the direction pass (clears P.counters first); one doubling
// round P.round from (P.q, P.s) into (P.q_next, P.s_next); the region out of the final planes; the stream network's count pass +
// the scan above over stream_waves() + 1 totals, and its emit pass into P.segments / P.stream_accumulation or P.prims
struct DrainParams;
hipError_t launch_drain_direction(const DrainParams &p, hipStream_t stream);
hipError_t launch_drain_round(const DrainParams &p, hipStream_t stream);
hipError_t launch_drain_write(const DrainParams &p, hipStream_t stream);
hipError_t launch_stream_count(const DrainParams &p, void *scan_tmp, size_t scan_bytes, hipStream_t stream);
hipError_t launch_stream_emit(const DrainParams &p, hipStream_t stream);
// drainage through depressions (f3d_fill.h, f3d_fill.hip): z, W0 and every tile dirty (clears P.counters first); one round
// P.round of the fill's relaxation over the tiles dirty in plane P.round & 1; T0 and the tiles that hold an undrained sample;
// one round of the flats'; the direction pass over P.fill_W / P.fill_T in place of launch_drain_direction (clears P.counters
// first); the filled samples and the largest T into the counters; the region out of the planes
struct FillParams;
hipError_t launch_fill_init(const FillParams &p, hipStream_t stream);
hipError_t launch_fill_relax(const FillParams &p, hipStream_t stream);
hipError_t launch_flat_init(const FillParams &p, hipStream_t stream);
hipError_t launch_flat_relax(const FillParams &p, hipStream_t stream);
hipError_t launch_fill_direction(const DrainParams &p, hipStream_t stream);
hipError_t launch_fill_stats(const FillParams &p, hipStream_t stream);
hipError_t launch_fill_write(const FillParams &p, hipStream_t stream);
hipError_t launch_ray_batch(const RayBatchParams &p, hipStream_t stream);
hipError_t launch_query(const QueryParams &p, hipStream_t stream);  // ray queries on a live session (f3d_query.h), 64 rays a workgroup
hipError_t launch_raster(const RasterParams &p, hipStream_t stream);  // DEM visibility rasters (f3d_raster.h), 64 consecutive samples a workgroup
hipError_t launch_horizon(const HorizonParams &p, hipStream_t stream);  // horizon rasters (f3d_horizon.h), one lane a DEM sample
hipError_t launch_irradiation(const IrradiationParams &p, hipStream_t stream);  // irradiation rasters (f3d_irradiation.h), 64 consecutive samples a workgroup
hipError_t launch_clearance(const ClearanceParams &p, hipStream_t stream);  // clearance rasters (f3d_clearance.h), one lane a DEM sample
hipError_t launch_umbra(const UmbraParams &p, hipStream_t stream);  // shadow-depth rasters (f3d_umbra.h), one lane a DEM sample
hipError_t launch_leaf_build(const PyramidBuildParams &p, hipStream_t stream);
hipError_t launch_level_build(const LevelBuildParams &p, hipStream_t stream);
hipError_t launch_band_build(const BandBuildParams &p, hipStream_t stream);
// far-horizon table of the IBL rays (f3d_cone.h): block level and block counts for a cell grid; the build (terrain
// must hold layout, bands, origin and spacing); table = bx * bz * 8 floats
void horizon_table_dims(uint32_t cell_w, uint32_t cell_h, uint32_t *level, uint32_t *bx, uint32_t *bz);
hipError_t launch_horizon_build(const TerrainDev &terrain, float *table, hipStream_t stream);

}  // namespace f3d
