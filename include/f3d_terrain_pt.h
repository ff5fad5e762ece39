/* include/f3d_terrain_pt.h -- C ABI of libf3dhip.so
 *
 * MI355X-native (gfx950, HIP) replacement for ONE path of forge3d: the PROMETHEUS
 * terrain path tracer behind `forge3d.hybrid_render_terrain_reference`.  These entry
 * points are what the reference's FFI for this path would bind (INTEGRATION.md shows
 * the Rust `extern "C"` block and the PyO3 shim a forge3d maintainer would add).
 * Plain pointers and sizes only; no torch / HIP types in any signature (streams and
 * device buffers travel as `void*`).  All functions are blocking unless stated and
 * thread-compatible (no hidden process-wide state besides the HIP primary context).
 *
 * Status codes: 0 ok; 1 value error (-> Python ValueError); 2 render error
 * (reference RenderError::Render -> RuntimeError "[Render] Render error: ...");
 * 3 upload error (RenderError::Upload); 4 device error (no GPU / HIP failure --
 * there is NO CPU fallback: without a usable gfx950 device every compute entry
 * point fails with status 4).
 */
#ifndef F3D_TERRAIN_PT_H
#define F3D_TERRAIN_PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever a struct of this header changes size or layout.  Every struct that has grown
 * (or may grow) carries its own size as its FIRST member; the caller sets it to sizeof(the struct it was compiled
 * against) and the library refuses a size it does not know (status 1) instead of reading past the caller's struct.
 *   1  round 1: f3d_terrain_ref_desc without `atmosphere`, no struct_size members
 *   2  round 2: + f3d_terrain_ref_desc.atmosphere (binary-incompatible, unversioned -- the reason for this scheme)
 *   3  round 3: + struct_size first in f3d_terrain_ref_desc / f3d_session_opts / f3d_wf_scene (and in the new
 *               f3d_composite_desc, f3d_aether_ref_desc), f3d_abi_version(); f3d_wf_scene + terrain, hair, medium;
 *               new entry points: peer halos (f3d_session_halo_*, f3d_session_enqueue_batch_strip),
 *               f3d_session_set_accumulation, f3d_smoke_step, f3d_smoke_composite, f3d_aether_reference_render
 *   4  round 4: + f3d_session_halo_stats / f3d_halo_stats, f3d_session_halo_probe modes 2 and 3 (no existing struct
 *               changed: a caller built against version 3 keeps working)
 *   5  round 5: + f3d_session_row_costs, f3d_session_primary_start, f3d_smoke_set_stream, f3d_smoke_wait_fields_read; the
 *               smoke entry points return without waiting when their results stay on the device and no time is asked for;
 *               f3d_wf_scene + primary_start at its end (no existing signature changed)
 *   6  round 6: + f3d_smoke_seq_* (a smoke sequence behind a handle: its streams, its ordering, its scratch).  The handle-less
 *               smoke entry points are synchronous again, as in ABI 4, unless the thread has called f3d_smoke_set_stream --
 *               which, with f3d_smoke_wait_fields_read, stays for this one revision as a shim over the thread's default
 *               context.  No struct changed: a caller built against version 3, 4 or 5 keeps working.
 *      since:   entry points with structs of their own are added without a bump and detected by their symbol (the session
 *               updates, queries, rasters, drape and paint; f3d_session_contours, f3d_session_paint_contours; f3d_session_drainage,
 *               f3d_session_streams, f3d_session_paint_streams; f3d_session_fill and the FILL flag of those three) */
#define F3D_ABI_VERSION 6u
#define F3D_STATUS_OK 0
#define F3D_STATUS_VALUE 1
#define F3D_STATUS_RENDER 2
#define F3D_STATUS_UPLOAD 3
#define F3D_STATUS_DEVICE 4

/* EarthModel / RefractionModel of reference src/geo/refraction.rs:15-43 */
#define F3D_EARTH_FLAT 0
#define F3D_EARTH_SPHERE 1
#define F3D_EARTH_ELLIPSOID 2
#define F3D_REFRACTION_NONE 0
#define F3D_REFRACTION_BENNETT 1
#define F3D_REFRACTION_SAEMUNDSSON 2
#define F3D_REFRACTION_EFFECTIVE_RADIUS 3

/* AETHER LUT payload handed to the aerial-perspective post: the reference's AtmosphereLutHandle
 * (src/core/atmosphere/runtime.rs:38-89; payload layout src/core/atmosphere/precomputed.rs:5-25) as plain host
 * pointers.  Tables are RGBA16F bit patterns, x fastest: transmittance [height][mu], accumulated scattering
 * [height * nu_count + nu][mu_sun][mu_view], aerial [height][mu_view][distance] (rgb = 0, a = mean transmittance). */
typedef struct f3d_aether_luts {
    const uint16_t *transmittance, *accumulated_scattering, *aerial;
    uint32_t transmittance_mu, transmittance_height;
    uint32_t scattering_mu_view, scattering_mu_sun, scattering_height, scattering_nu;
    uint32_t aerial_distance, aerial_mu_view, aerial_height;
    /* AtmosphereConfig, src/core/atmosphere/bake.rs:131-162 */
    float turbidity, ozone_du, mie_g, bottom_radius_m, top_radius_m, rayleigh_scale_height_m, mie_scale_height_m,
        max_aerial_distance_m, ground_albedo;
    uint32_t scattering_orders;
} f3d_aether_luts;

/* Mirrors TerrainReferenceDesc (reference
 * src/path_tracing/hybrid_compute/render_terrain.rs:239-282) plus the earth /
 * refraction parameters the PyO3 seam parses (src/py_functions/path_tracing/
 * terrain_reference.rs:295-312).  All pointers are HOST pointers that are only read
 * during the call. */
typedef struct f3d_terrain_ref_desc {
    uint32_t struct_size; /* = sizeof(f3d_terrain_ref_desc) of the caller's header (see F3D_ABI_VERSION) */
    const float *heights; /* (dem_height, dem_width) row-major f32 */
    uint32_t dem_width, dem_height;
    float spacing_x, spacing_z;
    float exaggeration;
    float albedo[3];
    float cam_origin[3], cam_look_at[3], cam_up[3];
    float fov_y_deg, exposure;
    float sun_azimuth_deg, sun_elevation_deg, sun_intensity;
    float sun_color[3];
    double observer_latitude_deg, observer_longitude_deg;
    int32_t earth_model;      /* F3D_EARTH_* */
    int32_t refraction_model; /* F3D_REFRACTION_* */
    double sphere_radius_m, refraction_k, pressure_mbar, temperature_c;
    const float *env_map; /* (env_height, env_width, 3) or NULL */
    uint32_t env_width, env_height;
    float env_intensity;
    const float *mesh_vertices; /* (mesh_vertex_count, 3) or NULL */
    uint32_t mesh_vertex_count;
    const uint32_t *mesh_indices; /* mesh_index_count entries, 3 per triangle, or NULL */
    uint32_t mesh_index_count;
    uint32_t width, height;
    uint32_t seed, spp, max_frames, min_frames;
    float variance_threshold;
    /* TerrainReferenceDesc::atmosphere (render_terrain.rs:265): NULL = no aerial perspective; else the converged
     * accumulation goes through the AETHER post (aether_post.rs, prometheus_aerial.wgsl) before the resolve. */
    const f3d_aether_luts *atmosphere;
} f3d_terrain_ref_desc;

/* Mirrors TerrainReferenceOutput (render_terrain.rs:285-299).  The four image
 * buffers are CALLER-allocated host memory; the library never frees or retains
 * them. */
typedef struct f3d_terrain_ref_out {
    uint8_t *rgba; /* (height, width, 4) */
    float *albedo; /* (height, width, 3) */
    float *normal; /* (height, width, 3) */
    float *depth;  /* (height, width), qNaN on miss */
    uint32_t frames;
    float variance;
    int32_t converged;
    uint64_t peak_host_visible_bytes;
    uint64_t minmax_pyramid_bytes;
    uint64_t gpu_resource_bytes;
    double loop_seconds;     /* accumulation loop only (device time, host clock) */
    double setup_seconds;    /* pyramid build + uploads + G-buffer pass */
    double readback_seconds; /* resolve + copies back */
} f3d_terrain_ref_out;

/* Replaces `_forge3d.hybrid_render_terrain_reference`
 * (reference src/py_functions/path_tracing/terrain_reference.rs:221-457 ->
 * HybridPathTracer::render_terrain_reference, render_terrain.rs:563-1434). */
int f3d_terrain_ref_render(const f3d_terrain_ref_desc *desc, f3d_terrain_ref_out *out, char *err,
                           size_t errlen);

/* ---- session API: the same render, device-resident and steppable -------------
 * Used by bench.py (inputs resident in HBM before the timed region) and by the
 * row-strip multi-GPU driver (forge3d_amd/distributed.py).  A session owns the
 * pixel rows [row_begin, row_end) of the full width x height image; RNG and all
 * state are keyed by full-image coordinates, so any partition reproduces the
 * single-GPU image. */
typedef struct f3d_session f3d_session;

#define F3D_FRAMES_IN_FLIGHT_AUTO 0xFFFFFFFFu
typedef struct f3d_session_opts {
    uint32_t struct_size; /* = sizeof(f3d_session_opts) of the caller's header */
    int32_t device;      /* HIP device ordinal, -1 = current */
    void *stream;        /* hipStream_t to enqueue on, NULL = the null stream */
    uint32_t row_begin;  /* first owned image row */
    uint32_t row_end;    /* one past the last owned row; 0 = height */
    uint64_t memory_budget_bytes; /* 0 = 512 MiB (reference MEMORY_BUDGET_LIMIT) */
    int32_t kernel_variant;       /* 0 = default.  A/B switches as decimal fields (forge3d_amd.session.kernel_variant() builds one
                                   * from names, describe_kernel_variant() reads one back):
                                   *   v % 1000              register budget of the frame kernel: 0 = 6 waves per SIMD (80 VGPRs);
                                   *                         104 = 4 waves (1 sample lane), 105 = 5 waves (4 sample lanes): the two
                                   *                         occupancy A/Bs profiles/README.md still cites; anything else is refused
                                   *   (v / 1000) % 10       tile -> XCD map: 0 / 2 rows dealt round-robin + longest-first dispatch
                                   *                         (default), 1 consecutive tiles, 3 contiguous bands, 4 = 2 without longest-first
                                   *   (v / 10000) % 100     lanes with a queued leaf that trigger a drain (0 = 64: only a full FIFO does)
                                   *   (v / 1000000) % 10    sample lanes per pixel: 1, 2, 4, 8; 0 = automatic (a non-zero register
                                   *                         budget with 0 here selects the 1-lane kernel)
                                   *   (v / 10000000) % 100  ray sharing: deal the IBL rays when at most this many lanes still march
                                   *                         (0 = 16; 64 = from the first step)
                                   * e.g. 4000105 = 4 sample lanes at 5 waves per SIMD; 8001000 = 8 lanes, consecutive tiles */
    /* Optional caller-owned DEVICE buffers (NULL -> the library allocates).  The
     * strip driver allocates these as torch tensors so RCCL can move them.
     *   reservoirs[2]: ping-pong packed reservoirs, each (rows + 8) * width * 16 B,
     *                  local row r holds image row row_begin - 4 + r;
     *   stats:         4 x u32 {max m2 bits, nonfinite flag, any_valid flag, bad_reservoir flag}. */
    void *ext_reservoirs[2];
    void *ext_stats;
    /* Band pipelining: the strip is cut into `bands` horizontal bands (0 = automatic: 1 for strips that fill
     * the chip, several for thin multi-GPU strips) whose launches go round-robin to `band_streams` internal
     * HIP streams (0 = automatic); band b of frame f + 1 waits only for bands b - 1, b, b + 1 of frame f (the
     * spatial reuse reads -3 .. +4 rows), so consecutive frames overlap and a thin strip is no longer bound by the
     * latency of one wave's ray chain.  Results do not depend on either number. */
    uint32_t bands;
    uint32_t band_streams;
    /* Acceleration structure of the optional triangle mesh: 0 = automatic (host SAH unless F3D_MESH_BVH=lbvh is
     * set in the environment), 1 = binned-SAH build on the host (reference accel::build_bvh, src/accel/sah_cpu.rs),
     * 2 = linear BVH built on the GPU (reference src/accel/lbvh_gpu: Morton codes, radix sort, Karras topology,
     * bottom-up refit).  Images do not depend on the choice. */
    uint32_t mesh_builder;
    /* Frames in flight: 0 / 1 = every frame is one fused launch (the default).  N >= 2: the session keeps a record
     * buffer for up to N frames (32 B x spp x pixels each, counted against memory_budget_bytes; N is lowered to what
     * fits) and f3d_session_enqueue_frames traces N frames in ONE launch -- what a frame traces does not depend on
     * the frames before it -- and then runs the cheap ordered half (reservoir chain, accumulation) per frame.  No
     * per-frame tail: the way thin multi-GPU strips stay throughput-bound.  Results do not depend on N.
     * F3D_FRAMES_IN_FLIGHT_AUTO: 16 for images too small to fill the chip with one frame, else 0 (what
     * f3d_terrain_ref_render uses).  f3d_session_frames_in_flight reports the effective value. */
    uint32_t frames_in_flight;
} f3d_session_opts;

int f3d_session_create(const f3d_terrain_ref_desc *desc, const f3d_session_opts *opts,
                       f3d_session **session, char *err, size_t errlen);
void f3d_session_destroy(f3d_session *session);

/* Enqueue accumulation frames [first_frame, first_frame + count) on the session
 * stream; asynchronous.  Multi-strip callers enqueue one frame at a time and
 * exchange the 4-row halos of reservoir buffer (frame & 1) between frames.  When
 * collect_stats_on_last != 0 the last frame of the batch also publishes the
 * convergence statistic read by f3d_session_window_stats. */
int f3d_session_enqueue_frames(f3d_session *session, uint32_t first_frame, uint32_t count,
                               int32_t collect_stats_on_last, char *err, size_t errlen);
/* Sessions with frames in flight, driven frame by frame (multi-GPU strips exchange halos between merges): trace
 * frames [first_frame, first_frame + count), count <= frames in flight, then merge each of them in order. */
int f3d_session_enqueue_trace(f3d_session *session, uint32_t first_frame, uint32_t count, char *err, size_t errlen);
int f3d_session_enqueue_merge(f3d_session *session, uint32_t frame, int32_t collect_stats, char *err, size_t errlen);
uint32_t f3d_session_frames_in_flight(f3d_session *session);
/* The batch size f3d_session_enqueue_frames would trace next at `frame` with `remaining` frames to go (short batches
 * for the first frames, then frames_in_flight): what a frame-by-frame driver passes to f3d_session_enqueue_trace. */
uint32_t f3d_session_trace_batch(f3d_session *session, uint32_t frame, uint32_t remaining);
/* Diagnostics (synchronises): pixel-frames traced a second time because the sun direction their frame head read was
 * mispredicted (see frames_in_flight); a handful per frame after the first two. */
int f3d_session_retraced_pixels(f3d_session *session, uint64_t *total);
/* One frame in two steps, for strips of a multi-GPU job: part 1 = the strip's EDGE bands (they contain the
 * first and last 4 pixel rows, the halo a neighbouring strip needs; on return the session stream is ordered
 * after them), part 2 = the interior bands.  The caller starts the halo exchange between the two, so that it
 * overlaps the interior.  Same result as f3d_session_enqueue_frames(frame, 1). */
int f3d_session_enqueue_frame_part(f3d_session *session, uint32_t frame, uint32_t part, int32_t collect_stats,
                                   char *err, size_t errlen);
/* Variance gate input for the window that ends after `frames` frames
 * (render_terrain.rs:1206-1231): synchronises the stream, returns max m2 over the
 * owned pixels (NOT yet divided by n-1) and whether a non-finite m2 was seen. */
int f3d_session_window_stats(f3d_session *session, float *max_m2, int32_t *nonfinite, char *err,
                             size_t errlen);
/* Device pointer + byte size of the halo rows of reservoir buffer `which` (0/1):
 * side 0 = the f3d_halo_rows() owned rows at the top (to send up), 1 = the owned rows at the
 * bottom (to send down), 2 = halo above the strip (to receive), 3 = halo below. */
int f3d_session_halo(f3d_session *session, int32_t which, int32_t side, void **ptr, uint64_t *bytes);
/* ---- peer halos: the strips of one node without the host or a collective in the frame chain --------------------
 * The classic strip loop (forge3d_amd/distributed.py) posts an RCCL send / recv pair from Python after every frame.
 * Here a strip PULLS its neighbours' edge rows itself: every session keeps a counter "frames merged" in device memory;
 * after a frame the library launches k_halo_pull, which raises that counter (it runs behind the frame's kernels) and
 * waits -- on the device -- until the neighbour's counter says its frame is done, then copies the neighbour's 4 edge
 * rows (peer memory mapped with hipIpcOpenMemHandle, read over xGMI with cache-bypassing loads) into the strip's own
 * halo rows.  Only READS cross the link and every strip writes nothing but its own memory, so no cache of another
 * device can hold a stale line.  f3d_session_enqueue_batch_strip enqueues a whole window of frames that way in one
 * call; RCCL is left with the per-window all-reduce and the final gather.
 *   f3d_session_halo_export   what a neighbour needs to map this strip (the session must own its reservoirs: no
 *                             ext_reservoirs); plain bytes, moved between the ranks by any means (all_gather)
 *   f3d_session_halo_connect  side 0 = the strip above (smaller rows), 1 = the strip below; peer = its export
 *   f3d_session_halo_probe    link check before the first frame: mode 0 stores `nonce` into this strip's counter block the
 *                             way the frame counter is stored, mode 1 reads the neighbours' words back (seen[0] = above,
 *                             seen[1] = below; 0 where there is no neighbour) with the loads the pull uses.  With a barrier
 *                             of the caller's between the two, a neighbour whose word does not read back (no peer access
 *                             between the devices, a stale mapping) is found before a frame depends on it
 *                             Modes 2 / 3 do the same with a REAL block: mode 2 fills this strip's two edge blocks of
 *                             reservoir buffer 0 with a pattern of `nonce` (a many-workgroup kernel, as the frame kernels
 *                             leave their rows) and publishes the nonce behind it; mode 3 (seen[0] / seen[1] = the nonces the
 *                             strips above / below published) waits for them on the device, pulls both blocks with the frame
 *                             loop's own kernel and compares their sums with the pattern's: seen[side] = 1 / 0, status 4 if a
 *                             block is not what its owner wrote.  Mode 4 clears reservoir buffer 0 again -- only after EVERY
 *                             strip has finished mode 3 (a barrier of the caller's: a neighbour may still be pulling this
 *                             strip's rows), and before any strip renders (another barrier)
 *   f3d_session_halo_status   device-side wait time-outs of the LAST f3d_session_enqueue_batch_strip (a dead neighbour must
 *                             not hang the GPU: a wait gives up after F3D_HALO_TIMEOUT_MS, default 20 000, and counts here;
 *                             a strip that has timed out stops pulling for the rest of that call -- its halo rows are stale --
 *                             and the caller turns a non-zero count into an error on every rank)
 *   f3d_session_halo_stats    how long this strip's pulls stood waiting for its neighbours since the last reset
 * Frame numbers of a connected session only rise: f3d_session_enqueue_batch_strip refuses a frame it has enqueued before
 * (the neighbours' counters are never cleared). */
typedef struct f3d_halo_stats {
    uint32_t reset;            /* in: 1 = clear the wait times and the pull count after reading them */
    uint32_t frames_published; /* this strip's frame counter */
    uint32_t timeouts, pulls;  /* waits that gave up (last call); neighbour blocks pulled */
    double wait_ms[2];         /* total device time the pulls waited for the strip above / below */
    double longest_wait_ms;    /* longest single wait */
    double timeout_ms;         /* the limit in force */
} f3d_halo_stats;
int f3d_session_halo_stats(f3d_session *session, f3d_halo_stats *out, char *err, size_t errlen);
typedef struct f3d_halo_export {
    uint8_t handle[3][64]; /* hipIpcMemHandle_t of reservoir buffer 0, 1 and of the counter block */
    uint64_t offset[3];    /* byte offset of the object inside the exported allocation */
    uint64_t address[3];   /* the objects' addresses in the exporting process (what a neighbour of the SAME process uses) */
    uint32_t rows, width;  /* owned rows of the strip, image width */
    int32_t device;        /* HIP device ordinal of the exporting process */
    uint32_t pid;          /* exporting process: a process cannot open its own handles */
} f3d_halo_export;
int f3d_session_halo_export(f3d_session *session, f3d_halo_export *out, char *err, size_t errlen);
int f3d_session_halo_connect(f3d_session *session, int32_t side, const f3d_halo_export *peer, char *err, size_t errlen);
int f3d_session_halo_probe(f3d_session *session, int32_t mode, uint32_t nonce, uint32_t *seen, char *err, size_t errlen);
int f3d_session_halo_status(f3d_session *session, uint32_t *timeouts, char *err, size_t errlen);
/* Frames [first, first + count) of a connected strip: per frame the frame's kernels (fused, or trace batch + merge with
 * frames in flight), the counter, the pull of both neighbours' rows.  One call, no host synchronisation. */
int f3d_session_enqueue_batch_strip(f3d_session *session, uint32_t first_frame, uint32_t count, int32_t collect_stats_on_last,
                                    char *err, size_t errlen);
/* Final resolve (last spatial reuse pass, reservoir validity, Reinhard + f16 + u8
 * quantisation, AOV conversion) and copy of the owned rows into host buffers that
 * cover ONLY the strip ((rows, width, C) each).  frames = accumulated frame count. */
int f3d_session_resolve(f3d_session *session, uint32_t frames, uint8_t *rgba, float *albedo,
                        float *normal, float *depth, int32_t *any_valid_reservoir, char *err,
                        size_t errlen);
/* Composition hook: replace the session's accumulated radiance sums by caller-supplied ones ((rows, width, 4) f32 host
 * memory: rgb = sums over `frames` frames, a ignored); the next f3d_session_resolve(frames) then tone-maps -- and, with
 * desc.atmosphere, sends through the AETHER post -- THAT radiance over the session's own depth / G-buffer.  How
 * BASELINE.json configs[2] combines the PBR tracer's multi-bounce radiance over the DEM (f3d_wavefront.h terrain
 * primitive) with the atmosphere post: forge3d_amd.offline.render_terrain_gi. */
int f3d_session_set_accumulation(f3d_session *session, const float *sums_rgba, char *err, size_t errlen);
/* Same, but leaves the results in caller-owned DEVICE buffers (for an RCCL gather). */
int f3d_session_resolve_device(f3d_session *session, uint32_t frames, void *d_rgba, void *d_albedo,
                               void *d_normal, void *d_depth, char *err, size_t errlen);
/* Host wall time of f3d_session_create by phase, ms: out[0] total, [1] validation + uniforms, [2] hashing the DEM (scene
 * cache key), [3] DEM upload, [4] acceleration-table build (synchronised), [5] mesh / environment / atmosphere uploads and
 * the mesh BVH, [6] allocation + clears of the per-pixel state, [7] enqueueing the G-buffer and certificate passes (their
 * device time is NOT in it: the call returns with them in flight).  [3] and [4] are 0 for a DEM the scene cache holds. */
#define F3D_SETUP_PHASES 8
int f3d_session_setup_ms(f3d_session *session, double *out, uint32_t count);
/* ---- re-arm: another render on a live session ---------------------------------------------------------------
 * What a new sun, seed, exposure, IBL intensity or frame budget changes, without a new session: the uniforms, the
 * per-pixel sun-ray certificates (recomputed from the resident G-buffer, the camera rays are not traced again), the
 * AETHER record's sun terms, and the per-render state (accumulation, Welford, both reservoir buffers with their halo
 * rows -- caller-owned ones included --, head records, tile costs, stats), cleared as a new session has them.  Camera,
 * DEM and exaggeration (see f3d_session_reterrain), spacing, mesh (see f3d_session_remesh), environment map, image size, strip rows, spp, earth / refraction model and
 * atmosphere LUTs stay the session's; observer latitude / longitude, pressure and temperature are re-armable (they
 * only enter the curvature of the secondary rays).  The next frames render exactly what a new session created with
 * these values renders.  Added without an ABI version bump (no existing struct or signature changed): a binding
 * detects the feature by the symbol f3d_session_rearm. */
typedef struct f3d_session_rearm_desc {
    uint32_t struct_size; /* = sizeof(f3d_session_rearm_desc) of the caller's header */
    float sun_azimuth_deg, sun_elevation_deg, sun_intensity;
    float sun_color[3];
    float exposure, env_intensity;
    uint32_t seed, max_frames, min_frames;
    float variance_threshold;
    double observer_latitude_deg, observer_longitude_deg, pressure_mbar, temperature_c;
} f3d_session_rearm_desc;
/* Validates with the create's code and messages (a refused descriptor leaves the session unchanged and usable), then
 * enqueues the re-arm pass on the session stream behind everything enqueued so far (band streams included) and
 * returns without waiting: frames, a resolve, a re-arm and the next frames may be enqueued back to back.  Allocates
 * nothing.  Refused (status 1) for a session with connected peer halos (their frame counters only rise). */
int f3d_session_rearm(f3d_session *session, const f3d_session_rearm_desc *desc, char *err, size_t errlen);
/* The accumulation / convergence-window / resolve / readback loop of f3d_terrain_ref_render on a live whole-image
 * session (f3d_terrain_ref_render is create + this loop + destroy): the same outputs, timings and errors; the frame
 * budget is the create's or the last re-arm's.  Blocking.  Once per create or re-arm (a second call without a re-arm in
 * between is refused, status 1: the accumulation it would continue is spent). */
int f3d_session_render(f3d_session *session, f3d_terrain_ref_out *out, char *err, size_t errlen);
/* Diagnostics (synchronises): content hashes of the sun-ray (out[0]) and primary-ray (out[1]) certificates. */
int f3d_session_certificates(f3d_session *session, uint64_t out[2]);
/* Diagnostics (synchronises): the deep-sky blocks of the session -- 8 x 8 pixel blocks whose pixels, and every pixel
 * within 4 of them, hold the sky certificate; a frame only accumulates there.  out = {blocks of the strip, deep blocks,
 * pixels that hold the sky certificate, pixels in deep blocks}.  0 deep blocks for a session whose frames use no such
 * table: an environment map, a mesh walk, one sample lane, frames in flight, more than one band. */
int f3d_session_sky_blocks(f3d_session *session, uint32_t out[4]);
/* ---- re-aim: a re-arm under a new camera ------------------------------------------------------------------------
 * What a new camera changes on top of a re-arm, still without a new session: the camera uniforms (all of them, the
 * pixel cone included), and everything the create's G-buffer pass writes -- normals and hit kind, depth, primary-ray
 * certificates (f3d_session_primary_start keeps returning the same pointer: its contents are the new view's after the
 * pass), sun-ray certificates.  One pass (k_reaim) traces the centre rays again, computes each sun certificate once and
 * clears the per-render state as the re-arm pass does; the longest-first tile order restarts from image order.  The
 * AETHER post reads the camera height and the pixel rays from the uniforms at resolve time, so it follows.  DEM and
 * exaggeration (see f3d_session_reterrain), spacing, mesh (see f3d_session_remesh), environment map, image size, strip rows and spp stay the session's.  The next frames
 * render exactly what a new session created with this camera and these values renders.  No ABI version bump: detected by
 * the symbol f3d_session_reaim. */
typedef struct f3d_session_reaim_desc {
    uint32_t struct_size; /* = sizeof(f3d_session_reaim_desc) of the caller's header */
    float cam_origin[3], cam_look_at[3], cam_up[3];
    float fov_y_deg;
    f3d_session_rearm_desc arm; /* everything a re-arm takes, same meaning (its struct_size is checked as well) */
} f3d_session_reaim_desc;
/* Same contract as f3d_session_rearm: validated by the create's code with its messages (a degenerate camera is refused
 * with the create's text and status; the session stays unchanged and usable), asynchronous on the session stream behind
 * everything enqueued so far, allocates nothing, works on the owned rows of a strip session, refused (status 1) for a
 * session with connected peer halos.  The setup_seconds of the f3d_session_render that follows is the host time of this
 * call plus that render's wait for the pass; it is not reported as zero. */
int f3d_session_reaim(f3d_session *session, const f3d_session_reaim_desc *desc, char *err, size_t errlen);
/* ---- re-mesh: a re-aim under a moved or another mesh -----------------------------------------------------------------
 * What a new mesh changes on top of a re-aim, still without a new session: the geometry standing on the terrain, and
 * with it everything the re-aim pass recomputes (centre hits, normals, depth, both certificates).  Two paths:
 *   mesh_indices == NULL   positions only, the REFIT path: mesh_vertex_count must be the session's.  The vertices are
 *     uploaded in stream order and the session's BVH is refitted on the GPU -- triangles gathered again in leaf order,
 *     scene bounds and the build's padding recomputed on the device, leaf boxes, then inner boxes bottom-up; the tree's
 *     topology stays, so large motion costs walk time, never the image.  Asynchronous on the session stream behind
 *     everything enqueued so far, no wait for the device.  The FIRST refit gives the session its own vertices, leaf-order
 *     triangles and nodes (the cached mesh other sessions share is never written; the indices stay shared) and the refit's
 *     tables: only that call allocates, against memory_budget_bytes (too small: refused, status 2); gpu_resource_bytes
 *     then exceeds a fresh session's by those tables and never grows again.
 *   mesh_indices != NULL   another mesh (any counts), the create's path with the session's builder: mesh cache, host SAH
 *     or LBVH build; may wait and allocate like a create; the old mesh is released once the work enqueued before the call
 *     has finished; gpu_resource_bytes equals a fresh session's.  Also the way to a fresh tree when motion has degraded a
 *     refitted one: pass the same indices again.
 * Validated by the create's code with its messages and statuses (mesh checks included; a non-finite vertex: "mesh
 * vertices contain non-finite values", status 2); a refusal leaves the session unchanged, usable and rendering the old
 * mesh.  Refused with status 1: a session created without a mesh, a vertex count other than the session's without
 * mesh_indices, connected peer halos, a session whose occlusion rays march a mesh grid (F3D_MESH_FUSED builds).  The
 * next frames render exactly what a new session created with this mesh, this camera and these values renders.  No ABI
 * version bump: detected by the symbol f3d_session_remesh. */
typedef struct f3d_session_remesh_desc {
    uint32_t struct_size;         /* = sizeof(f3d_session_remesh_desc) of the caller's header */
    const float *mesh_vertices;   /* HOST, (mesh_vertex_count, 3), read during the call only */
    uint32_t mesh_vertex_count;
    const uint32_t *mesh_indices; /* NULL = the session's topology (positions only: the refit path); else another mesh */
    uint32_t mesh_index_count;
    f3d_session_reaim_desc aim;   /* camera + everything a re-arm takes, same meaning */
} f3d_session_remesh_desc;
int f3d_session_remesh(f3d_session *session, const f3d_session_remesh_desc *desc, char *err, size_t errlen);
/* ---- re-terrain: a re-aim under new DEM samples -------------------------------------------------------------------------
 * What new heights change on top of a re-aim, still without a new session: the ground itself -- a time-lapse, an erosion
 * or excavation step, a cut-and-fill edit, another exaggeration -- and with it everything the re-aim pass recomputes
 * (centre hits, normals, depth, both certificates).  The update is a BLOCK of samples: width x height at DEM sample
 * (x0, y0), row-major with pitch = width; the whole DEM is the block (0, 0, dem_width, dem_height).  It is uploaded in
 * stream order into a staging buffer of the session and two kernels patch the session's OWN leaf table and band tables
 * (f3d_retable.h): the cells with a corner in the block get exactly those corners replaced by height * exaggeration and
 * their level-0 band, then every band level is rebuilt over the block's footprint from the level below -- the bits the
 * create's builders produce, two launches whatever the DEM's size, no raw-height copy, no node table.  Asynchronous on
 * the session stream behind everything enqueued so far, no wait for the device (a block above 8 MiB goes through the
 * library's two 4 MiB pinned staging buffers more than once: its third chunk waits for its first).  The FIRST call gives the session its
 * own tables (filled from the scene-cache entry by device copies; that entry, which other sessions and later creates
 * share, is never written); only that call, and a call whose block is larger than any before (the staging buffer grows),
 * allocate, against memory_budget_bytes (too small: refused, status 2); gpu_resource_bytes then exceeds a fresh session's
 * by the staging buffer.
 * exaggeration: 0 keeps the session's; another value rescales every sample, so it is accepted only with the whole DEM.
 * DEM size and spacing stay the session's.  Validated by the create's code with its messages and statuses (a non-finite
 * sample: "terrain heightfield contains non-finite samples", status 3; an exaggeration or a camera the create refuses:
 * its text, status 2); a refusal leaves the session unchanged, usable and rendering the old terrain.  Refused with status
 * 1: another struct_size, an empty block or one that leaves the DEM, a new exaggeration with a partial block, connected
 * peer halos, a session whose occlusion rays march a mesh grid (F3D_MESH_FUSED builds), a session that built the opt-in
 * far-horizon table (F3D_IBL_HORIZON=1: it would be stale).  The next frames render exactly what a new session created
 * with the resulting DEM, this camera and these values renders.  No ABI version bump: detected by the symbol
 * f3d_session_reterrain. */
typedef struct f3d_session_reterrain_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_reterrain_desc) of the caller's header */
    const float *heights;        /* HOST, the block, row-major, pitch = width; read during the call only */
    uint32_t width, height;      /* of the block, >= 1 */
    uint32_t x0, y0;             /* DEM sample of the block's first sample */
    float exaggeration;          /* 0: keep; another value only with the whole DEM */
    f3d_session_reaim_desc aim;  /* camera + everything a re-arm takes, same meaning */
} f3d_session_reterrain_desc;
int f3d_session_reterrain(f3d_session *session, const f3d_session_reterrain_desc *desc, char *err, size_t errlen);
/* ---- ray queries: pick, line of sight, ground --------------------------------------------------------------------------
 * A live session holds the only current copy of its scene -- the ground after a re-terrain (no raw-height copy of the DEM is
 * kept), the mesh after a re-mesh, the camera after a re-aim.  A query asks that scene a question with the frame kernels' own
 * device functions, one lane a ray (k_query, csrc/f3d_query.h), and changes nothing a frame launch reads: it is allowed at
 * any time, between frames and on sessions with connected peer halos.
 *   mode 0  closest hit  the caller's ray as given -> the reference's intersect_hybrid (curvature off, mesh and terrain)
 *   mode 1  occlusion    the caller's ray as given -> the any-hit march of the shadow / IBL rays; CURVED: with the sun rays'
 *                        curvature policy.  Answers `kind` only (any other output: refused, status 1): an any-hit walk stops
 *                        at the first surface it meets, its t is not the closest hit's
 *   mode 2  pixels       the centre ray of pixel (gx, gy) of the session's CURRENT camera (origin = camera, tmin 1e-3, tmax 1e30):
 *                        the bits the G-buffer pass stores in the depth and normal AOVs.  Full-image coordinates: a strip session
 *                        answers for any pixel of the image.  A pixel outside the image: refused (status 1) before anything
 *                        is enqueued (DEVICE_POINTERS: its lane answers a miss -- the host never sees the pixels)
 * In modes 0 and 1 t is in units of |direction|: nothing is normalised.  Answers do not depend on the form of the mesh's tree.
 * TERRAIN_ONLY leaves the mesh out ("clamp to ground": an object must not land on itself).
 * A BAD ray -- a non-finite component, a direction whose squared length is not a positive finite f32, tmax <= tmin -- is
 * never refused and never marched: its lane answers a miss before any walk starts, in the host and the device form alike.
 * Ordering: the kernel is enqueued on the session stream behind everything enqueued so far (band streams included), as a
 * re-arm is: a query right after a re-aim / re-mesh / re-terrain sees the new scene, no host wait in between.
 *   host pointers (default)  blocking.  Rays go up and results come down through the library's pinned staging pair in stream
 *       order (no plain copy races frames in flight), via a scratch buffer of the session: 80 bytes a ray (32 in, 48 out,
 *       whichever outputs are asked for), allocated when a larger count than any before arrives -- against
 *       memory_budget_bytes (too small: status 2, session unchanged) and counted in gpu_resource_bytes
 *   DEVICE_POINTERS          rays and every output are device memory (rays 16-byte aligned); nothing is copied or allocated.
 *       The call returns when the kernel has finished, or -- NO_WAIT -- with it in flight: the caller orders by the stream
 *       the session was created on
 * count == 0 is a successful no-op.  No ABI version bump: detected by the symbol f3d_session_query. */
#define F3D_QUERY_CLOSEST 0u
#define F3D_QUERY_OCCLUSION 1u
#define F3D_QUERY_PIXELS 2u
#define F3D_QUERY_TERRAIN_ONLY 1u
#define F3D_QUERY_CURVED 2u
#define F3D_QUERY_DEVICE_POINTERS 4u
#define F3D_QUERY_NO_WAIT 8u
#define F3D_QUERY_SCRATCH_BYTES_PER_RAY 80u
typedef struct f3d_session_query_desc {
    uint32_t struct_size; /* = sizeof(f3d_session_query_desc) of the caller's header */
    uint32_t mode;        /* F3D_QUERY_CLOSEST / _OCCLUSION / _PIXELS */
    uint32_t flags;       /* F3D_QUERY_TERRAIN_ONLY | _CURVED (mode 1 only) | _DEVICE_POINTERS | _NO_WAIT (with _DEVICE_POINTERS only) */
    uint32_t count;
    const void *rays;     /* modes 0 / 1: count x 8 f32 (origin xyz, tmin, direction xyz, tmax) -- the layout of f3d_terrain_trace_batch;
                             mode 2: count x 2 u32 (gx, gy), full-image coordinates */
    /* outputs, each may be NULL */
    uint32_t *kind;       /* 0 miss, 1 terrain, 2 mesh; mode 1: 0 clear / 1 occluded */
    float *t;             /* ray parameter; qNaN 0x7fc00000 on a miss (what the depth AOV holds) */
    float *normal;        /* count x 3; zeros on a miss */
    float *position;      /* count x 3: origin + t * direction as closest_hit forms it; zeros on a miss */
    uint32_t *primitive;  /* terrain: cx | cz << 16 of the hit cell; mesh: the triangle's index in the caller's mesh_indices; miss: 0xFFFFFFFF */
    float *direction;     /* count x 3, mode 2 only: the centre ray's direction */
} f3d_session_query_desc;
int f3d_session_query(f3d_session *session, const f3d_session_query_desc *desc, char *err, size_t errlen);
/* ---- DEM visibility rasters: viewshed, sun mask, sun hours ----------------------------------------------------------------
 * One question of EVERY DEM sample of a region, the rays built on the device from the terrain the session holds and marched
 * with the occlusion query's any-hit march (k_raster, csrc/f3d_raster.h): no ray list goes up, one bit per sample per target
 * comes down.  All arithmetic is f32, one rounding per operation.  Sample n = r * cols + c of the region is DEM sample
 * (row0 + r, col0 + c); its ray starts at (origin_x + col * spacing_x, height * exaggeration + lift, origin_z + row * spacing_z)
 * (each plane one fma).  A target is four f32 (x, y, z, w):
 *   F3D_RASTER_TOWARD_POINT     (x, y, z) is a world position (a viewshed's observer): the ray is origin -> position, t in
 *                               [0, 1].  CURVED on a scene with earth curvature lowers the direction's y by
 *                               hd2 * inv_two_r_prime (hd2 the squared horizontal distance), so that the curved march meets the
 *                               position's own height above its datum at t = 1.  w > 0: a maximum horizontal distance,
 *                               hd2 > w * w answers 0 without a march
 *   F3D_RASTER_ALONG_DIRECTION  (x, y, z) is the ray's direction as given (a sun mask), t in [0, 1e30]; w is reserved: 0
 * SESSION_SUN (ALONG_DIRECTION, target_count 0, targets NULL): one target, the direction the frames' sun rays use NOW.
 * Bit 1 = visible / lit; 0 = blocked, beyond the distance limit, or a ray the occlusion query would not march (a non-finite
 * component, a zero direction: an observer exactly on the lifted sample).
 *   masks  target_count x ceil(rows * cols / 64) uint64: bit n of target k is bit (n & 63) of word k * words + (n >> 6); pad bits 0
 *   count  rows * cols uint32: the number of targets whose bit is 1
 * Either may be NULL, not both.  TERRAIN_ONLY, CURVED, DEVICE_POINTERS, NO_WAIT and the ordering on the session stream are
 * the ray query's; nothing a frame launch reads is written.
 *   host pointers (default)  blocking; targets go up and the outputs come down through the pinned staging pair via a scratch
 *       buffer of the session (16 bytes a target + the outputs asked for), grown only for a larger call than any before --
 *       against memory_budget_bytes (too small: status 2, session unchanged).  Non-finite targets: refused
 *   DEVICE_POINTERS          targets (16-byte aligned), masks and count are device memory; nothing is copied or allocated
 * Refused (status 1, session unchanged): an unknown mode or flag, a region that is empty or reaches outside the DEM, a
 * non-finite lift, SESSION_SUN with targets or toward a point, NO_WAIT without DEVICE_POINTERS, both outputs NULL.
 * target_count == 0 without SESSION_SUN is a successful no-op.  No ABI version bump: detected by the symbol f3d_session_raster. */
#define F3D_RASTER_TOWARD_POINT 0u
#define F3D_RASTER_ALONG_DIRECTION 1u
#define F3D_RASTER_TERRAIN_ONLY 1u
#define F3D_RASTER_CURVED 2u
#define F3D_RASTER_DEVICE_POINTERS 4u
#define F3D_RASTER_NO_WAIT 8u
#define F3D_RASTER_SESSION_SUN 16u
typedef struct f3d_session_raster_desc {
    uint32_t struct_size;  /* = sizeof(f3d_session_raster_desc) of the caller's header */
    uint32_t mode;         /* F3D_RASTER_TOWARD_POINT / _ALONG_DIRECTION */
    uint32_t flags;        /* F3D_RASTER_TERRAIN_ONLY | _CURVED | _DEVICE_POINTERS | _NO_WAIT | _SESSION_SUN */
    uint32_t row0;         /* the region, in DEM samples: rows [row0, row0 + rows), columns [col0, col0 + cols) */
    uint32_t col0;
    uint32_t rows;
    uint32_t cols;
    float lift;            /* added to every sample's height (a viewshed's target height, a shadow mask's bias) */
    uint32_t target_count;
    uint32_t reserved;     /* 0 */
    const float *targets;  /* target_count x 4 f32 */
    uint64_t *masks;       /* target_count x ceil(rows * cols / 64), or NULL */
    uint32_t *count;       /* rows * cols, or NULL */
} f3d_session_raster_desc;
int f3d_session_raster(f3d_session *session, const f3d_session_raster_desc *desc, char *err, size_t errlen);
/* ---- horizon rasters: horizon slopes and sky-view factor ----------------------------------------------------------------------
 * For every DEM sample of a region and every azimuth, the slope under which the GROUND hides the sky (terrain only: a
 * session with a mesh answers for its terrain) -- one max-slope walk of the min/max pyramid per sample per azimuth
 * (k_horizon; the contract, the leaf's closed form and the bound are at the head of csrc/f3d_horizon.h).  The sample stands
 * on the lifted lattice point o of the visibility rasters (lift >= 0); an azimuth is a horizontal direction (dx, dz), two
 * f32 used as given; with p(t) = (o.x + t dx, o.z + t dz) and y the bilinear surface,
 *     H = sup over t > 0, p(t) inside the footprint, of (y(p(t)) - k t^2 - o.y) / t
 * k = (dx^2 + dz^2) inv_two_r_prime with CURVED on a scene with earth curvature, else 0: (dx, H, dz) is the grazing direction
 * of the visibility rasters' rays under the same flag.  For a unit (dx, dz) H is the tangent of the horizon's elevation.
 * No terrain along the azimuth (a border sample looking outward; a line along the DEM's last row or column, where the
 * march finds no cell either): -inf.  lift == 0 includes the limit t -> 0+.  All arithmetic is f32, one rounding per operation.
 *   horizon   azimuth_count x rows * cols f32: plane k is azimuth k, sample n = r * cols + c
 *   sky_view  rows * cols f32: 1 - (sum_k s_k) / azimuth_count, s_k = max(h, 0) / sqrt(1 + h^2), h = H_k / sqrt(dx_k^2 + dz_k^2)
 *             (the horizontal-surface sky-view factor; -inf and NaN azimuths contribute 0), summed in f32 for k = 0, 1, ...
 * Either may be NULL, not both; with horizon NULL nothing of size azimuth_count x rows * cols is written or allocated.
 * CURVED, DEVICE_POINTERS, NO_WAIT and the ordering on the session stream are the raster's; nothing a frame launch reads is
 * written.
 *   host pointers (default)  blocking; staged through the visibility rasters' scratch buffer (the outputs asked for + 8 bytes
 *       an azimuth), grown only for a larger call than any before, against memory_budget_bytes (too small: status 2, session
 *       unchanged).  A non-finite or zero (dx, dz): refused
 *   DEVICE_POINTERS          azimuths (8-byte aligned), horizon and sky_view are device memory; nothing is copied or allocated.
 *       A non-finite or zero (dx, dz): that plane is NaN
 * A walk that exceeds its step cap (no DEM does) writes NaN for that azimuth of that sample.
 * Refused (status 1, session unchanged): an unknown flag, NO_WAIT without DEVICE_POINTERS, a region that is empty or reaches
 * outside the DEM, a non-finite or negative lift, azimuth_count 0 or above F3D_HORIZON_MAX_AZIMUTHS, NULL azimuths, both
 * outputs NULL.  No ABI version bump: detected by the symbol f3d_session_horizon. */
#define F3D_HORIZON_CURVED 2u
#define F3D_HORIZON_DEVICE_POINTERS 4u
#define F3D_HORIZON_NO_WAIT 8u
#define F3D_HORIZON_MAX_AZIMUTHS 256u
typedef struct f3d_session_horizon_desc {
    uint32_t struct_size;   /* = sizeof(f3d_session_horizon_desc) of the caller's header */
    uint32_t flags;         /* F3D_HORIZON_CURVED | _DEVICE_POINTERS | _NO_WAIT */
    uint32_t row0;          /* the region, in DEM samples: rows [row0, row0 + rows), columns [col0, col0 + cols) */
    uint32_t col0;
    uint32_t rows;
    uint32_t cols;
    float lift;             /* added to every sample's height, >= 0 */
    uint32_t azimuth_count; /* 1 .. F3D_HORIZON_MAX_AZIMUTHS */
    const float *azimuths;  /* azimuth_count x 2 f32: (dx, dz) */
    float *horizon;         /* azimuth_count x rows * cols, or NULL */
    float *sky_view;        /* rows * cols, or NULL */
    uint32_t reserved;      /* 0 */
} f3d_session_horizon_desc;
int f3d_session_horizon(f3d_session *session, const f3d_session_horizon_desc *desc, char *err, size_t errlen);
/* ---- irradiation rasters: beam energy over a sun track ------------------------------------------------------------------------
 * For every DEM sample of a region, the energy the direct beam delivers over a set of sun positions: each position weighted
 * by its irradiance and by the cosine of incidence on the local slope, counted where the visibility rasters' ray toward it
 * is unblocked (k_irradiation; the contract is at the head of csrc/f3d_irradiation.h).  All arithmetic is f32, one rounding
 * per operation, no fma.  The sample stands on the lifted lattice point o of the visibility rasters.  Its gradient (gx, gz) is
 * the central difference of the heights the session holds (exaggeration applied), one-sided on the DEM's border, over the
 * lattice's own plane positions; q = (gx gx + gz gz) + 1; the unit normal is (-gx, 1, -gz) / sqrt(q).  HORIZONTAL: gx = gz = 0
 * (the beam on a horizontal plane).  A direction is four f32 (x, y, z, weight): toward the sun, as given (need not be unit),
 * and a weight >= 0 (W/m^2 x hours, say).  With l2 = (x x + y y) + z z, m = (y - gx x) - gz z and c = m / sqrt(q l2), the term
 * counts when weight > 0, c > 0, the ray (o, (x, y, z), t in [0, 1e30]) is one the occlusion query marches and it is unblocked:
 *   energy  rows * cols f32: the sum of weight * c over the terms that count, added in f32 for k = 0, 1, ...
 *   count   rows * cols uint32: the number of terms that count
 *   normal  rows * cols x 3 f32: the unit normal
 * A facet turned away from the sun, a zero weight and a refused direction add nothing and march no ray.  Any output may be
 * NULL, not all; with normal alone direction_count may be 0 and nothing marches.  TERRAIN_ONLY, CURVED, DEVICE_POINTERS,
 * NO_WAIT and the ordering on the session stream are the raster's; nothing a frame launch reads is written.
 *   host pointers (default)  blocking; staged through the visibility rasters' scratch buffer (the outputs asked for + 16 bytes
 *       a direction), grown only for a larger call than any before, against memory_budget_bytes (too small: status 2, session
 *       unchanged).  A non-finite component or a negative weight: refused
 *   DEVICE_POINTERS          directions (16-byte aligned), energy, count and normal are device memory; nothing is copied or
 *       allocated.  A non-finite component or a negative weight: that term is 0
 * Refused (status 1, session unchanged): an unknown flag, reserved != 0, NO_WAIT without DEVICE_POINTERS, a region that is
 * empty or reaches outside the DEM, a non-finite lift, all outputs NULL, direction_count 0 with energy or count asked for,
 * NULL directions with direction_count > 0.  No ABI version bump: detected by the symbol f3d_session_irradiation. */
#define F3D_IRRADIATION_TERRAIN_ONLY 1u
#define F3D_IRRADIATION_CURVED 2u
#define F3D_IRRADIATION_DEVICE_POINTERS 4u
#define F3D_IRRADIATION_NO_WAIT 8u
#define F3D_IRRADIATION_HORIZONTAL 16u
typedef struct f3d_session_irradiation_desc {
    uint32_t struct_size;     /* = sizeof(f3d_session_irradiation_desc) of the caller's header */
    uint32_t flags;           /* F3D_IRRADIATION_TERRAIN_ONLY | _CURVED | _DEVICE_POINTERS | _NO_WAIT | _HORIZONTAL */
    uint32_t row0;            /* the region, in DEM samples: rows [row0, row0 + rows), columns [col0, col0 + cols) */
    uint32_t col0;
    uint32_t rows;
    uint32_t cols;
    float lift;               /* added to every sample's height (the shadow rays' bias) */
    uint32_t direction_count;
    const float *directions;  /* direction_count x 4 f32: (x, y, z, weight) */
    float *energy;            /* rows * cols, or NULL */
    uint32_t *count;          /* rows * cols, or NULL */
    float *normal;            /* rows * cols x 3, or NULL */
    uint32_t reserved;        /* 0 */
} f3d_session_irradiation_desc;
int f3d_session_irradiation(f3d_session *session, const f3d_session_irradiation_desc *desc, char *err, size_t errlen);
/* ---- clearance rasters: the height needed to be seen ---------------------------------------------------------------------------
 * For every DEM sample of a region and every observer, how far above the GROUND a target over that sample must stand for
 * the observer to see it -- the "above ground level" output of a GIS viewshed: one pass is the viewshed for every target
 * height at once (terrain only: a session with a mesh answers for its terrain).  One bounded max-slope walk of the min/max
 * pyramid per sample per observer, from the observer (k_clearance; the contract, the leaf's closed form and the bound are at
 * the head of csrc/f3d_clearance.h).  The sample's lattice point g = (g.x, h, g.z) is the visibility rasters' with lift 0; an
 * observer is four f32 (x, Y, z, w) as a TOWARD_POINT target of f3d_session_raster, w > 0 a maximum horizontal distance.  With
 * dx = x - g.x, dz = z - g.z, hd2 = dx dx + dz dz, k = hd2 inv_two_r_prime with CURVED on a scene with earth curvature (else 0),
 * p(t) = (g.x + t dx, g.z + t dz) and y the bilinear surface,
 *     L* = sup over t in (0, 1), p(t) inside the footprint, of (y(p(t)) - t Y) / (1 - t) + k t - h
 * is the smallest lift at which the TOWARD_POINT raster's ray from the sample is unblocked, and the value is max(L*, +0).
 *   +inf  hd2 > w w; the observer under the surface; the sample straight over the observer (hd2 == 0 and Y < h)
 *   0     the ground itself shows: no terrain between, or none high enough; hd2 == 0 and Y >= h
 *   NaN   a walk that exceeds its step cap (no DEM does); a non-finite observer component in the device form
 * All arithmetic is f32, one rounding per operation.
 *   height  observer_count x rows * cols f32: plane k is observer k, sample n = r * cols + c
 *   lowest  rows * cols f32: the minimum over the observers ("seen by any of them"), NaN planes ignored
 * Either may be NULL, not both; with height NULL nothing of size observer_count x rows * cols is written or allocated.
 * CURVED, DEVICE_POINTERS, NO_WAIT and the ordering on the session stream are the raster's; nothing a frame launch reads is
 * written.
 *   host pointers (default)  blocking; staged through the visibility rasters' scratch buffer (the outputs asked for + 16 bytes
 *       an observer), grown only for a larger call than any before, against memory_budget_bytes (too small: status 2, session
 *       unchanged).  A non-finite observer component or a negative w: refused
 *   DEVICE_POINTERS          observers (16-byte aligned), height and lowest are device memory; nothing is copied or allocated.
 * Refused (status 1, session unchanged): an unknown flag, reserved != 0, NO_WAIT without DEVICE_POINTERS, a region that is
 * empty or reaches outside the DEM, observer_count 0, NULL observers, both outputs NULL.  No ABI version bump: detected by
 * the symbol f3d_session_clearance. */
#define F3D_CLEARANCE_CURVED 2u
#define F3D_CLEARANCE_DEVICE_POINTERS 4u
#define F3D_CLEARANCE_NO_WAIT 8u
typedef struct f3d_session_clearance_desc {
    uint32_t struct_size;     /* = sizeof(f3d_session_clearance_desc) of the caller's header */
    uint32_t flags;           /* F3D_CLEARANCE_CURVED | _DEVICE_POINTERS | _NO_WAIT */
    uint32_t row0;            /* the region, in DEM samples: rows [row0, row0 + rows), columns [col0, col0 + cols) */
    uint32_t col0;
    uint32_t rows;
    uint32_t cols;
    uint32_t observer_count;  /* >= 1 */
    const float *observers;   /* observer_count x 4 f32: (x, Y, z, w) */
    float *height;            /* observer_count x rows * cols, or NULL */
    float *lowest;            /* rows * cols, or NULL */
    uint32_t reserved;        /* 0 */
} f3d_session_clearance_desc;
int f3d_session_clearance(f3d_session *session, const f3d_session_clearance_desc *desc, char *err, size_t errlen);
/* ---- shadow-depth rasters: the height needed to be lit ------------------------------------------------------------------------
 * For every DEM sample of a region and every direction toward a light, how far above the GROUND a point over that sample must
 * stand to be lit from it -- the mounting height at which a panel or a mast catches the sun, the top of the terrain's shadow
 * volume: one pass is the sun mask for every lift at once (terrain only: a session with a mesh answers for its terrain).  One
 * bounded walk of the min/max pyramid per sample per direction, from the sample (k_umbra; the contract, the leaf's closed form
 * and the bound are at the head of csrc/f3d_umbra.h).  The sample's lattice point g = (g.x, h, g.z) is the visibility rasters'
 * with lift 0; a direction is four f32 (dx, dy, dz, w), used as given, as an ALONG_DIRECTION target of f3d_session_raster; w is
 * reserved: 0.  With k = (dx dx + dz dz) inv_two_r_prime with CURVED on a scene with earth curvature (else 0),
 * p(t) = (g.x + t dx, g.z + t dz) and y the bilinear surface,
 *     L* = max(+0, sup over t > 0, p(t) inside the footprint, of y(p(t)) - k t^2 - dy t - h)
 * is the smallest lift at which the ALONG_DIRECTION raster's ray from the sample is unblocked under the same flag.  dy <= 0 is
 * legal: the footprint is finite.
 *   0     the ground itself is lit: no terrain along the direction, or none high enough; dx == dz == 0 and dy > 0
 *   +inf  dx == dz == 0 and dy < 0
 *   NaN   a walk that exceeds its step cap (no DEM does); in the device form a non-finite component, a zero direction, w != 0
 * All arithmetic is f32, one rounding per operation.
 *   depth    direction_count x rows * cols f32: plane k is direction k, sample n = r * cols + c
 *   deepest  rows * cols f32: the maximum over the directions (above it the sample is lit from all of them), NaN planes ignored
 * Either may be NULL, not both; with depth NULL nothing of size direction_count x rows * cols is written or allocated.
 * SESSION_SUN (direction_count 0, directions NULL): one plane, the direction the frames' sun rays use NOW, as
 * F3D_RASTER_SESSION_SUN.  CURVED, DEVICE_POINTERS, NO_WAIT and the ordering on the session stream are the raster's; nothing a
 * frame launch reads is written.
 *   host pointers (default)  blocking; staged through the visibility rasters' scratch buffer (the outputs asked for + 16 bytes
 *       a direction), grown only for a larger call than any before, against memory_budget_bytes (too small: status 2, session
 *       unchanged).  A non-finite component, a zero direction or w != 0: refused
 *   DEVICE_POINTERS          directions (16-byte aligned), depth and deepest are device memory; nothing is copied or allocated.
 * Refused (status 1, session unchanged), in this order: an unknown flag, reserved != 0, NO_WAIT without DEVICE_POINTERS,
 * SESSION_SUN with directions, a region that is empty or reaches outside the DEM, direction_count 0 without SESSION_SUN, NULL
 * directions, both outputs NULL.  No ABI version bump: detected by the symbol f3d_session_umbra. */
#define F3D_UMBRA_CURVED 2u
#define F3D_UMBRA_DEVICE_POINTERS 4u
#define F3D_UMBRA_NO_WAIT 8u
#define F3D_UMBRA_SESSION_SUN 16u
typedef struct f3d_session_umbra_desc {
    uint32_t struct_size;      /* = sizeof(f3d_session_umbra_desc) of the caller's header */
    uint32_t flags;            /* F3D_UMBRA_CURVED | _DEVICE_POINTERS | _NO_WAIT | _SESSION_SUN */
    uint32_t row0;             /* the region, in DEM samples: rows [row0, row0 + rows), columns [col0, col0 + cols) */
    uint32_t col0;
    uint32_t rows;
    uint32_t cols;
    uint32_t direction_count;  /* >= 1; 0 with SESSION_SUN */
    uint32_t reserved;         /* 0 */
    const float *directions;   /* direction_count x 4 f32: (dx, dy, dz, 0); NULL with SESSION_SUN */
    float *depth;              /* direction_count x rows * cols, or NULL */
    float *deepest;            /* rows * cols, or NULL */
} f3d_session_umbra_desc;
int f3d_session_umbra(f3d_session *session, const f3d_session_umbra_desc *desc, char *err, size_t errlen);
/* ---- drape: an image laid over the terrain, per-texel albedo ---------------------------------------------------------------
 * What an image changes on top of a re-aim, still without a new session: the albedo of TERRAIN hits.  The drape is
 * image[rows][cols] of linear RGB reflectances, f32, row-major, `channels` (3 or 4; a fourth channel is ignored) values a
 * texel; image row 0 lies on DEM row 0 and image column 0 on DEM column 0 -- the heightmap's own orientation.  It replaces
 * f3d_terrain_ref_desc.albedo for terrain hits only: mesh hits keep (0.7, 0.7, 0.8), the sky is untouched.  All arithmetic
 * is f32, one rounding per operation.  A terrain hit at world (x, z) has the DEM-sample coordinates
 *     fx = (x - origin_x) / spacing_x, fz = (z - origin_z) / spacing_z        (origin: -(dem - 1) * spacing / 2, as everywhere)
 * and the texel coordinates tx = fx * scale_x + offset_x, tz = fz * scale_z + offset_z (finite numbers, scales non-zero; an
 * image that covers the DEM's extent edge to edge: scale = cols / (dem_width - 1), offset = -0.5; texel centres on the
 * corresponding fraction of samples: scale = (cols - 1) / (dem_width - 1), offset = 0).
 *   F3D_DRAPE_NEAREST   texel clamp(floor(t + 0.5), 0, n - 1) per axis
 *   F3D_DRAPE_BILINEAR  clamp to edge: i0 = floor(t), f = t - i0, taps clamp(i0), clamp(i0 + 1); every lerp is a + f * (b - a),
 *                       along x first, then along z -- a constant image samples to exactly that constant
 * Texels are stored as binary16 RGBA (8 bytes, rounded to nearest even as the RGBA16F AOVs are) in a buffer of the session:
 * rows * cols * 8 bytes, tracked in gpu_resource_bytes and checked against memory_budget_bytes (too small: status 2, the old
 * drape stays).  The frames sample it once per primary hit -- candidate weight, sun term and IBL term all take the sampled
 * albedo -- in a draped instantiation of the fused frame kernel; the albedo AOV of a terrain pixel is the drape at the centre
 * ray's hit point (the position f3d_session_query mode 2 reports for the pixel), rounded to half as before.
 *   image == NULL            removes the drape: every later output is bit-identical to a session that never had one
 *   F3D_DRAPE_PATCH          image overwrites the window rows [at_row, at_row + rows) x columns [at_col, at_col + cols) of the
 *                            session's drape (a time-lapse of imagery without uploading all of it again): the drape keeps its
 *                            size, filter and registration (the descriptor's are not read).  Refused (status 1) without a drape
 *                            or when the window does not fit
 *   host pointers (default)  the texels are looked at first: a non-finite, negative or > 65504 value in a read channel is
 *                            refused (status 3, "drape texels must be finite and >= 0 ...").  They go up through the pinned
 *                            staging pair in stream order, a slab of rows at a time via a scratch buffer of the session (at most
 *                            8 MiB or one row, grown only for a wider row than any before, tracked and budgeted), and k_drape_pack
 *                            rounds them into the drape.  The call returns once the image has been read; it does not wait
 *                            for the device
 *   F3D_DRAPE_DEVICE_POINTERS image is device memory; nothing is copied and nobody can look: k_drape_pack stores a value
 *                            that is non-finite, negative or > 65504 as 0.  The call returns when the kernel has finished, or
 *                            -- F3D_DRAPE_NO_WAIT, with DEVICE_POINTERS only -- with it in flight: the caller orders by the
 *                            stream the session was created on and keeps the image alive until the kernel has read it
 * An update like re-arm / re-aim / re-mesh / re-terrain: `aim` carries the camera and everything a re-arm takes, the render
 * restarts at frame 0, everything is validated by the create's code with its messages, every refusal comes before the first
 * change of the session, and all of it is enqueued on the session stream behind everything enqueued so far.  The next frames
 * render exactly what a new session draped the same way renders.  A drape survives the other four updates.
 * Refused with status 1: another struct_size, an unknown flag or filter, channels other than 3 or 4, an empty image or one
 * above 16384 texels a side, a non-finite registration number or a zero scale, NO_WAIT without DEVICE_POINTERS, connected
 * peer halos, a session with frames in flight, a register-budget A/B kernel variant (104, 4105).  A draped session renders
 * through the fused frame path (f3d_session_enqueue_frames, f3d_session_render): f3d_session_enqueue_trace / _merge,
 * _enqueue_frame_part and _enqueue_batch_strip refuse it (status 1).  No ABI version bump: detected by the symbol
 * f3d_session_drape. */
#define F3D_DRAPE_NEAREST 0u
#define F3D_DRAPE_BILINEAR 1u
#define F3D_DRAPE_DEVICE_POINTERS 4u
#define F3D_DRAPE_NO_WAIT 8u
#define F3D_DRAPE_PATCH 16u
#define F3D_DRAPE_MAX_SIDE 16384u
typedef struct f3d_session_drape_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_drape_desc) of the caller's header */
    uint32_t flags;              /* F3D_DRAPE_DEVICE_POINTERS | _NO_WAIT | _PATCH */
    const float *image;          /* rows x cols x channels f32, row-major; NULL removes the drape; read during the call only
                                    (NO_WAIT: until the kernel has run) */
    uint32_t rows, cols;         /* of the image (PATCH: of the window) */
    uint32_t channels;           /* 3 or 4 */
    uint32_t filter;             /* F3D_DRAPE_NEAREST / _BILINEAR */
    float scale_x, offset_x;     /* tx = fx * scale_x + offset_x */
    float scale_z, offset_z;     /* tz = fz * scale_z + offset_z */
    uint32_t at_row, at_col;     /* PATCH: the window's first texel in the session's drape; otherwise 0 */
    f3d_session_reaim_desc aim;  /* camera + everything a re-arm takes, same meaning */
} f3d_session_drape_desc;
int f3d_session_drape(f3d_session *session, const f3d_session_drape_desc *desc, char *err, size_t errlen);
/* Is the session draped?  info (may be NULL) = {rows, cols, filter, bytes of the drape buffer}; returns 1 / 0 (no session: 0). */
int f3d_session_draped(f3d_session *session, uint32_t info[4]);

/* ---- paint: vector features composited into the drape -----------------------------------------------------------------------
 * Roads, rivers, parcels, tracks, summit markers: points, line segments or triangles in world x-z, rasterised on the device
 * into the session's drape (the canvas), which the draped frames then sample as before.  No image crosses the bus: the call
 * uploads the primitives only.  The per-texel rule is the opening comment of csrc/f3d_paint.h -- f32, one rounding per
 * operation, independent of the tiling the device uses:
 *   lines      index pairs; a stroke of half-width half_width metres with round caps and joins and a one-texel coverage ramp
 *              (one texel = ramp = max(|spacing_x / scale_x|, |spacing_z / scale_z|) metres), colour and alpha lerped along it
 *   points     single indices; the segment with both ends equal: a disc of radius half_width
 *   triangles  index triples; coverage 1 or 0 at the texel centre with a top-left rule and edge functions that two triangles
 *              sharing an edge evaluate to the same bits (a mesh is watertight: no gap, no texel blended twice); zero-area
 *              triangles paint nothing; colour and alpha barycentric
 * A run of consecutive primitives whose FIRST vertices carry one feature id is one feature: per texel its primitive with the
 * highest coverage counts (ties: the lowest index), and it blends once,  dst += (opacity * alpha * cov) * (src - dst),  features
 * in list order.  feature == NULL: the whole call is one feature.  Texels stay binary16: they are read, blended in f32 and
 * written once per call; an untouched texel keeps its bits.
 * An update like f3d_session_drape: ordered on the session stream behind everything enqueued, the render restarts at frame 0
 * (aim: the camera and the re-armable members, as a re-aim takes them), every refusal comes before the first change, and the
 * drape keeps its size, filter and registration.  The call waits for the device twice, for two counters (the number of
 * (tile, primitive) pairs and of non-empty tiles), and returns with the paint kernel enqueued.
 * Refused with status 1: a session without a drape; unknown flags or primitive; an index count that is no multiple of the
 * primitive's (1, 2, 3) or zero; an index >= vertex_count; more than 2^24 primitives; a negative or non-finite half_width; an
 * opacity outside [0, 1]; peer halos.  Status 3 (a host scan of all vertices): a non-finite coordinate; a coordinate more than
 * 65536 texels (65536 ramp metres) from the terrain's centre, the world's origin -- the reach the f32 distances are sized for:
 * clip far geometry to the terrain's neighbourhood --; an RGBA outside [0, 1].
 * Status 2, the canvas unchanged: the primitive records (80 bytes each), the keys and the sort's storage do not fit
 * memory_budget_bytes -- session buffers, tracked in gpu_resource_bytes, sized exactly after the count pass, grown only, freed
 * with the drape.  The keys are sized after the count pass has run on the records' buffer: when THEY are refused that first
 * buffer may have grown (gpu_resource_bytes with it); the canvas, the render state and f3d_session_fingerprint are as before. */
#define F3D_PAINT_POINTS 0u
#define F3D_PAINT_LINES 1u
#define F3D_PAINT_TRIANGLES 2u
#define F3D_PAINT_MAX_PRIMITIVES 16777216u
typedef struct f3d_session_paint_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_paint_desc) of the caller's header */
    uint32_t flags;              /* none defined: 0 */
    uint32_t primitive;          /* F3D_PAINT_POINTS / _LINES / _TRIANGLES */
    uint32_t vertex_count;       /* N */
    const float *xz;             /* N x 2 f32: world x, z; host memory, read during the call only (as rgba, feature, indices) */
    const float *rgba;           /* N x 4 f32 in [0, 1]: linear RGB reflectance and alpha */
    const uint32_t *feature;     /* N feature ids, or NULL: one feature */
    const uint32_t *indices;     /* index_count indices into the vertices: 1 / 2 / 3 a primitive */
    uint32_t index_count;
    float half_width;            /* metres: half the stroke width, the disc's radius; checked, not used, for triangles */
    float opacity;               /* [0, 1] */
    f3d_session_reaim_desc aim;  /* camera + everything a re-arm takes, same meaning */
} f3d_session_paint_desc;
int f3d_session_paint(f3d_session *session, const f3d_session_paint_desc *desc, char *err, size_t errlen);
/* Diagnostics of the session's last paint call (tools/paint_time.py): ms = device time of {count pass + scan, emit + sort + run
 * list, paint kernel} from events on the session stream (waits for them); counts = {primitives, (tile, primitive) keys, tiles
 * painted}.  Either may be NULL.  Returns 1, or 0 when the session has not painted. */
int f3d_session_paint_stats(f3d_session *session, double ms[3], uint64_t counts[3]);
/* ---- contour lines: extracted, and painted into the drape, on the device ---------------------------------------------------
 * Marching squares over the cells of the session's terrain, as the leaf table holds it: heights are f32(h * exaggeration), the y
 * that a ground query returns, and `levels` are in that unit -- finite, strictly ascending, at most F3D_CONTOUR_MAX_LEVELS.  The
 * rule is the opening comment of csrc/f3d_contour.h (f32, one rounding per operation): the case of a cell is the sum of its
 * corners' bits (h >= level; h00 1, h10 2, h01 4, h11 8), the segment table and the fixed pairing of the two saddles are the
 * reference's contour_extract's, and a crossing belongs to its lattice EDGE -- the two cells sharing an edge compute the same
 * bits, so the ends of neighbouring segments are bit-identical and can be joined by comparing bits; a level through a sample
 * gives zero-length segments, which are emitted.  The region is a region of CELLS {row0, col0, rows, cols} of the
 * (dem_height - 1) x (dem_width - 1) grid.  Records come in "block order": blocks of 8 x 8 cells aligned to the cell grid,
 * row-major over blocks, cells row-major in a block, levels ascending in a cell, a case's segments in table order.
 *
 * f3d_session_contours is a query (ordered on the session stream behind everything enqueued; the render goes on): it writes the
 * first min(*total, capacity) records -- segments: 4 f32 (ax, az, bx, bz) in world x-z; level_index: the level's index in
 * `levels` -- and always *total, so a call with capacity 0 sizes the next.  levels and total are host memory; with
 * DEVICE_POINTERS segments (16-byte aligned) and level_index are device memory.  There is no NO_WAIT: the total crosses the bus.
 * Refused with status 1, in this order: the struct size; unknown flags; reserved != 0; an empty region; a region that leaves
 * the cell grid; NULL levels or level_count 0; more than F3D_CONTOUR_MAX_LEVELS; a non-finite level or levels not strictly
 * ascending; NULL total; capacity > 0 with NULL segments (segments or level_index with capacity 0 is legal; level_index may be
 * NULL); with DEVICE_POINTERS, segments not 16-byte aligned.  Status 2: the scratch (16 bytes a block, the levels, in the host
 * form the min(*total, capacity) records written -- not the capacity) does not fit memory_budget_bytes.  Both entry points answer
 * status 4 before any other check in a process without a HIP device.
 *
 * f3d_session_paint_contours is an update like f3d_session_paint (the render restarts at frame 0, aim as there): the segments
 * are emitted on the device straight into the session's paint buffer -- as `lines` of one feature with one colour, the bits
 * f3d_session_paint builds for the same segments -- and rasterised by the same kernels; *total is the number painted (0: the
 * drape keeps its bits).  Refused, in this order, the session and its drape unchanged: the struct size (its own, aim's, the
 * re-arm's), peer halos, then as above through NULL total (status 1); a session without a drape; half_width negative or
 * non-finite; opacity outside [0, 1]; rgba outside [0, 1]; a corner of the region more than 65536 texels of the drape from the
 * terrain's centre (status 3, as f3d_session_paint's reach); the re-arm's own refusals; and, after the count pass, more than
 * F3D_PAINT_MAX_PRIMITIVES segments (status 1) or buffers beyond memory_budget_bytes (status 2).
 * No ABI version bump: detected by the symbols f3d_session_contours and f3d_session_paint_contours. */
#define F3D_CONTOUR_DEVICE_POINTERS 4u
#define F3D_CONTOUR_MAX_LEVELS 65536u
typedef struct f3d_session_contours_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_contours_desc) of the caller's header */
    uint32_t flags;              /* F3D_CONTOUR_DEVICE_POINTERS */
    uint32_t row0, col0, rows, cols; /* the region, in cells */
    uint32_t level_count;
    uint32_t reserved;           /* 0 */
    const float *levels;         /* level_count f32, host memory, read during the call only */
    float *segments;             /* capacity x 4 f32, or NULL */
    uint32_t *level_index;       /* capacity u32, or NULL */
    uint64_t capacity;           /* records the outputs hold */
    uint64_t *total;             /* host memory: the number of segments of the region */
} f3d_session_contours_desc;
int f3d_session_contours(f3d_session *session, const f3d_session_contours_desc *desc, char *err, size_t errlen);
typedef struct f3d_session_paint_contours_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_paint_contours_desc) of the caller's header */
    uint32_t flags;              /* none defined: 0 */
    uint32_t row0, col0, rows, cols; /* the region, in cells */
    uint32_t level_count;
    uint32_t reserved;           /* 0 */
    const float *levels;         /* level_count f32, host memory, read during the call only */
    uint64_t *total;             /* host memory: the number of segments painted */
    float rgba[4];               /* [0, 1]: linear RGB reflectance and alpha of every segment */
    float half_width;            /* metres: half the stroke width */
    float opacity;               /* [0, 1] */
    f3d_session_reaim_desc aim;  /* camera + everything a re-arm takes, same meaning */
} f3d_session_paint_contours_desc;
int f3d_session_paint_contours(f3d_session *session, const f3d_session_paint_contours_desc *desc, char *err, size_t errlen);
/* ---- drainage: flow directions, flow accumulation, basins and the stream network, on the device ---------------------------------
 * Where water goes over the session's terrain as the leaf table holds it (heights f32(h * exaggeration), the y of a ground query).
 * The rule is the opening comment of csrc/f3d_drainage.h (f32, one rounding per operation): D8 -- the eight neighbours in the order
 * E, SE, S, SW, W, NW, N, NE = codes 0 .. 7 (+column east, +row south), slope = drop / run with run the spacing or, on a diagonal,
 * sqrt(spacing_x^2 + spacing_z^2); the steepest positive slope wins, ties go to the lowest code; a sample without one is a sink,
 * code 8 (pits, flats, the border's outlets).  Accumulation is the number of samples whose path passes through a sample, itself
 * included; the basin of a sample is the linear index (row * dem_width + column) of the sink its path ends in.  Without the
 * FILL flag (below) no depressions are filled and no flats resolved.  THE WHOLE DEM IS ROUTED BY EVERY CALL, from the tables as they are (nothing is kept between
 * calls; a re-terrain needs no invalidation): the region {row0, col0, rows, cols} of SAMPLES, as the visibility rasters', selects
 * what is written.  The accumulation is summed by path doubling, floor(log2(longest path)) + 1 rounds of integer atomics: the
 * results do not depend on the device's scheduling.  The scratch is the visibility rasters' buffer: 21 bytes a DEM sample (33
 * with FILL), plus, in the host forms, what is written.
 *
 * f3d_session_drainage is a query (ordered on the session stream behind everything enqueued; the render goes on): direction
 * (rows * cols u8), accumulation and basin (rows * cols u32 each), sample n = r * cols + c; each may be NULL.  stats (host memory,
 * 3 u32) is always written: the DEM's sinks, the doubling rounds that had a live sample, the longest path in steps.  ms (host
 * memory, 2 f64, or NULL): the host's clock to the device's end of the direction pass, then of the rounds.  With DEVICE_POINTERS
 * the three planes are device memory (accumulation and basin 4-byte aligned).  There is no NO_WAIT: a counter crosses the bus
 * after every round.  Refused with status 1, in this order: the struct size; unknown flags; reserved != 0; an empty region; a
 * region that leaves the DEM; NULL stats; with DEVICE_POINTERS, a misaligned plane; a DEM of more than 2^31 samples (the live
 * bit shares the pointer word; with it every DEM whose counts would not fit 32 bits).  Status 2: the scratch does not fit
 * memory_budget_bytes.
 *
 * f3d_session_streams is a query: every sample of the region that is no sink and has accumulation >= threshold (>= 1) gives one
 * segment from its own lattice point to its receiver's (which may lie outside the region), in row-major order of the region's
 * samples.  It writes the first min(*total, capacity) records -- segments: 4 f32 (ax, az, bx, bz) in world x-z; accumulation:
 * the sample's -- and always *total, so a call with capacity 0 sizes the next.  total is host memory; with DEVICE_POINTERS
 * segments (16-byte aligned) and accumulation are device memory.  Refused with status 1, in this order: the struct size; unknown
 * flags; reserved != 0; an empty region; a region that leaves the DEM; threshold 0; NULL total; capacity > 0 with NULL segments;
 * with DEVICE_POINTERS, segments not 16-byte aligned; more than 2^31 samples.  Status 2 as above (the host form's records are
 * sized by min(*total, capacity), not by the capacity).
 *
 * f3d_session_paint_streams is an update like f3d_session_paint_contours: the segments are emitted on the device straight into
 * the session's paint buffer -- as `lines` of one feature with one colour, the bits f3d_session_paint builds for the same
 * segments -- and rasterised by the same kernels; *total is the number painted (0: the drape keeps its bits).  Refused, in this
 * order, the session and its drape unchanged: the struct size (its own, aim's, the re-arm's), peer halos, then as above through
 * NULL total (status 1); a session without a drape; half_width negative or non-finite; opacity outside [0, 1]; more than 2^31
 * samples; rgba outside [0, 1]; the region, widened by one sample, more than 65536 texels of the drape from the terrain's
 * centre (status 3, as f3d_session_paint's reach); the re-arm's own refusals; and, after the count pass, more than
 * F3D_PAINT_MAX_PRIMITIVES segments (status 1) or buffers beyond memory_budget_bytes (status 2).
 * All three answer status 4 before any other check in a process without a HIP device.  No ABI version bump: detected by the
 * symbols f3d_session_drainage, f3d_session_streams and f3d_session_paint_streams.
 *
 * HYDROLOGICALLY CONDITIONED ROUTING: F3D_DRAINAGE_FILL (= F3D_STREAMS_FILL, accepted in `flags` of all three descriptors; their
 * members and every other bit's meaning are unchanged) routes over the FILLED surface instead, by the rule in the opening
 * comment of csrc/f3d_fill.h.  A sample on the DEM's first or last row or column is an outlet.  The filled surface W is z on
 * outlets and elsewhere the greatest solution of W(c) = max(z(c), min over the neighbours of W): the least height over all
 * paths to an outlet of the highest sample on the path, what priority-flood computes.  The flat distance T is 0 on outlets and
 * on samples with a strictly lower neighbour in W, elsewhere 1 + the least T among the neighbours of equal W.  The direction is
 * D8 on W; a sample without a positive slope that is no outlet goes to the lowest code with a smaller W, or an equal W and a
 * smaller T.  Every step lowers (W, T): the only sinks are outlets, every river reaches the border, the sinks' accumulations
 * still sum to the DEM's samples.  Both surfaces are fixed points of monotone relaxations that only select among the input
 * values: the bits do not depend on the device's scheduling.  Accumulation, basins, stats and the stream records keep their
 * meaning over the new receivers.  Detected by the symbol f3d_session_fill.
 *
 * f3d_session_fill is a query like f3d_session_drainage: of the region's samples, filled (W, f32), depth (W - z, one f32
 * subtraction: the lakes' water depth) and flat_distance (T, u32), rows * cols each, any of them NULL.  stats (host memory,
 * 4 u32, or NULL): the DEM's samples with W > z, the rounds of the fill pass, the rounds of the flat pass, the largest T.  ms
 * (host memory, 2 f64, or NULL): the host's clock to the device's end of the fill pass, then of the flat pass.  With
 * DEVICE_POINTERS the three planes are device memory, 4-byte aligned.  The scratch is 12 bytes a DEM sample plus, in the host
 * form, what is written.  Refused with status 1, in this order: the struct size; unknown flags; reserved != 0; an empty region;
 * a region that leaves the DEM; with DEVICE_POINTERS, a misaligned plane; a DEM of more than 2^31 samples.  Status 2: the
 * scratch does not fit memory_budget_bytes.  Status 4 before any other check in a process without a HIP device. */
#define F3D_DRAINAGE_DEVICE_POINTERS 4u
#define F3D_STREAMS_DEVICE_POINTERS 4u
#define F3D_DRAINAGE_FILL 8u
#define F3D_STREAMS_FILL 8u
#define F3D_FILL_DEVICE_POINTERS 4u
#define F3D_DRAINAGE_SINK 8u
typedef struct f3d_session_drainage_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_drainage_desc) of the caller's header */
    uint32_t flags;              /* F3D_DRAINAGE_DEVICE_POINTERS, F3D_DRAINAGE_FILL */
    uint32_t row0, col0, rows, cols; /* the region, in DEM samples */
    uint8_t *direction;          /* rows * cols codes 0 .. 8, or NULL */
    uint32_t *accumulation;      /* rows * cols, or NULL */
    uint32_t *basin;             /* rows * cols, or NULL */
    uint32_t *stats;             /* host memory, 3 u32: sinks, rounds, longest */
    double *ms;                  /* host memory, 2 f64, or NULL */
    uint32_t reserved;           /* 0 */
} f3d_session_drainage_desc;
int f3d_session_drainage(f3d_session *session, const f3d_session_drainage_desc *desc, char *err, size_t errlen);
typedef struct f3d_session_streams_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_streams_desc) of the caller's header */
    uint32_t flags;              /* F3D_STREAMS_DEVICE_POINTERS, F3D_STREAMS_FILL */
    uint32_t row0, col0, rows, cols; /* the region, in DEM samples */
    uint32_t threshold;          /* >= 1: the accumulation from which a sample is a stream */
    uint32_t reserved;           /* 0 */
    float *segments;             /* capacity x 4 f32, or NULL */
    uint32_t *accumulation;      /* capacity u32, or NULL */
    uint64_t capacity;           /* records the outputs hold */
    uint64_t *total;             /* host memory: the number of segments of the region */
} f3d_session_streams_desc;
int f3d_session_streams(f3d_session *session, const f3d_session_streams_desc *desc, char *err, size_t errlen);
typedef struct f3d_session_paint_streams_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_paint_streams_desc) of the caller's header */
    uint32_t flags;              /* F3D_STREAMS_FILL */
    uint32_t row0, col0, rows, cols; /* the region, in DEM samples */
    uint32_t threshold;          /* >= 1 */
    uint32_t reserved;           /* 0 */
    uint64_t *total;             /* host memory: the number of segments painted */
    float rgba[4];               /* [0, 1]: linear RGB reflectance and alpha of every segment */
    float half_width;            /* metres: half the stroke width */
    float opacity;               /* [0, 1] */
    f3d_session_reaim_desc aim;  /* camera + everything a re-arm takes, same meaning */
} f3d_session_paint_streams_desc;
int f3d_session_paint_streams(f3d_session *session, const f3d_session_paint_streams_desc *desc, char *err, size_t errlen);
typedef struct f3d_session_fill_desc {
    uint32_t struct_size;        /* = sizeof(f3d_session_fill_desc) of the caller's header */
    uint32_t flags;              /* F3D_FILL_DEVICE_POINTERS */
    uint32_t row0, col0, rows, cols; /* the region, in DEM samples */
    float *filled;               /* rows * cols f32: the filled surface W, or NULL */
    float *depth;                /* rows * cols f32: W - z, or NULL */
    uint32_t *flat_distance;     /* rows * cols u32: T, or NULL */
    uint32_t *stats;             /* host memory, 4 u32: filled samples, fill rounds, flat rounds, largest T; or NULL */
    double *ms;                  /* host memory, 2 f64, or NULL */
    uint32_t reserved;           /* 0 */
} f3d_session_fill_desc;
int f3d_session_fill(f3d_session *session, const f3d_session_fill_desc *desc, char *err, size_t errlen);
/* The drape's texels as f32 RGB in host memory, after everything enqueued on the session: region = {row0, col0, rows, cols} (NULL:
 * the whole drape), rgb_out = rows x cols x 3 f32.  What a composed map is saved with.  Status 1: no drape, a region that leaves it. */
int f3d_session_drape_read(f3d_session *session, const uint32_t region[4], float *rgb_out, char *err, size_t errlen);
/* Memory / layout diagnostics of a session. */
int f3d_session_info(f3d_session *session, uint64_t *gpu_resource_bytes, uint64_t *minmax_pyramid_bytes,
                     uint64_t *peak_host_visible_bytes, uint32_t *rows, uint32_t *width);
/* Average device time in ms of the `count` most recent frame-kernel launches,
 * measured with hipEvents recorded on the session stream around every launch when
 * timing is enabled (bench.py's roofline leg).  enable: 1 start, 0 stop. */
int f3d_session_kernel_timing(f3d_session *session, int32_t enable, double *avg_ms, uint32_t *launches);
/* Sample lanes per pixel the frame kernel of this session runs with (1, 2, 4 or 8); 0 on a NULL session. */
uint32_t f3d_session_sample_lanes(f3d_session *session);
/* (ABI 5) Cost of the session's last fused frame by image row (out[rows], rows = the session's; 100 MHz ticks of wave time,
 * a tile's duration spread over its rows): what the strip driver balances row strips on.  Synchronises the stream. */
int f3d_session_row_costs(f3d_session *session, float *out, uint32_t rows, char *err, size_t errlen);
/* (ABI 5) The session's primary-ray certificates (f3d_cone.h): a DEVICE pointer to rows x width records {f32 bits of t_clear,
 * u32 level}, written by the G-buffer pass the session's creation enqueued on its stream; NULL when the camera's pixels are too
 * wide for certificates.  Valid while the session lives; the call waits for the session's stream, so the records are written
 * when it returns.  The PBR path tracer takes it as f3d_wf_scene.primary_start (same camera, image size and heightfield). */
const void *f3d_session_primary_start(f3d_session *session);
/* Device memory the library has freed is kept for its next allocation of the same size (F3D_DEVICE_POOL_MB, default
 * 1024, 0 = off): a camera path or a smoke sequence allocates the same buffers frame after frame.  This hands everything
 * that is waiting back to the driver -- call it before another allocator (torch, RCCL) sizes large buffers on the device:
 * what the pool holds is invisible to them. */
void f3d_device_pool_trim(void);
/* Rows of neighbour state a strip keeps above and below its own (4: the spatial pass reaches -3 .. +4 rows); the halo
 * blocks of f3d_session_halo and the extra rows of ext_reservoirs are this many rows. */
uint32_t f3d_halo_rows(void);

/* Diagnostics: out[0..15] = hashes of everything a frame launch of this session reads.  [0] camera, [1] light,
 * [2] terrain scalars, [3] mesh scalars, [4] other scalars, [5] leaf table, [6] band tables, [7] mesh vertices,
 * [8] mesh indices, [9] BVH nodes, [10] BVH triangles, [11] environment, [12] G-buffer, [13] reservoirs,
 * [14] accumulation + Welford, [15] frame-head records.  Synchronises the session.  count >= 16.  A caller that passes
 * count >= 17 also gets [16] the drape (f3d_session_drape: its record without the device address, and its texels; 0 without
 * a drape); a caller that passes 16 is written 16 words as before. */
int f3d_session_fingerprint(f3d_session *session, uint64_t *out, uint32_t count);

/* Diagnostics (no ABI version bump: detected by the symbol): the mesh BVH this session's frame launches walk, read back from
 * the device as it is NOW -- the shared cache entry's tree, or the session's own copy once f3d_session_remesh has refitted
 * it.  info = {form, node_count, triangle_count, 0}; form 0: the session walks no tree (no mesh), 1: node_count records of
 * 32 bytes {f32 bmin[3], u32 skip, f32 bmax[3], u32 leaf} in threaded preorder (node i's first child is i + 1, skip = the
 * node after its subtree, leaf = 0 or (first triangle << 3) | count), 2: node_count records of 128 bytes {f32 lo_x[4],
 * hi_x[4], lo_y[4], hi_y[4], lo_z[4], hi_z[4], u32 leaf[4], first_child, inner, pad[2]} (slots [0, inner) are the records
 * first_child + slot, the others leaves or empty: both planes +inf, leaf 0).  Triangles: 3 x {f32 xyz, w} each in leaf
 * order, the original triangle index as the bits of corner 0's w.  nodes / tris NULL: the sizes only; otherwise exactly
 * node_count records and 3 * triangle_count corners are written, and a capacity below that is F3D_STATUS_VALUE.
 * Synchronises the session. */
int f3d_session_mesh_tree(f3d_session *session, uint32_t info[4], void *nodes, size_t node_capacity_bytes, void *tris,
                          size_t tri_capacity_bytes, char *err, size_t errlen);

/* Diagnostics (only in builds with -DF3D_WAVE_TIMES; F3D_STATUS_VALUE otherwise): every frame-kernel workgroup
 * writes its {start, end} wall clock (100 MHz ticks) to device_buffer[2 * workgroup]; NULL switches it off. */
int f3d_session_debug_wave_times(f3d_session *session, void *device_buffer);

/* ---- post filter ---------------------------------------------- */
/* Edge-aware a-trous denoiser: replaces forge3d.denoise.atrous_denoise
 * (reference python/forge3d/denoise.py:18-127).  color / albedo / normal: H x W x 3 f32,
 * depth: H x W f32; albedo, normal, depth may be NULL.  `out` (H x W x 3 f32) is caller-owned.
 * iterations < 1 runs one pass, like the reference. */
int f3d_atrous_denoise(const float *color, const float *albedo, const float *normal, const float *depth,
                       uint32_t width, uint32_t height, int32_t iterations, float sigma_color, float sigma_albedo,
                       float sigma_normal, float sigma_depth, float *out, char *err, size_t errlen);

/* ---- AETHER atmosphere LUT baker (the offline half) ------------------------------------
 * Replaces bake_atmosphere_luts (reference src/core/atmosphere/bake.rs:1481-1666; cargo feature `atmosphere-bake`,
 * single-thread host code there): the tables of an f3d_aether_luts for any AtmosphereConfig, not only the five shipped
 * turbidity anchors.  Outputs are RGBA16F bit patterns in the reference's layouts (x fastest): transmittance
 * [height][mu]; single and accumulated scattering [height][nu][mu_sun][mu_view]; aerial [height][mu_view][distance];
 * order_deltas[scattering_orders] = mean |field| of every order (AtmosphereLuts::order_deltas). */
typedef struct f3d_aether_bake_config { /* AtmosphereConfig + LutDimensions, bake.rs:32-42,132-144 */
    float turbidity, ozone_du, mie_g, bottom_radius_m, top_radius_m, rayleigh_scale_height_m, mie_scale_height_m,
        max_aerial_distance_m, ground_albedo;
    uint32_t scattering_orders; /* 2..8 */
    uint32_t transmittance_mu, transmittance_height, scattering_mu_view, scattering_mu_sun, scattering_height, scattering_nu,
        aerial_distance, aerial_mu_view, aerial_height; /* 2..256 each */
} f3d_aether_bake_config;
int f3d_aether_bake(const f3d_aether_bake_config *config, uint16_t *transmittance, uint16_t *single_scattering,
                    uint16_t *accumulated_scattering, uint16_t *aerial, float *order_deltas, double *seconds, char *err,
                    size_t errlen);

/* ---- smoke volume ray-marcher (BASELINE.json configs[4]) --------------------------
 * Replaces SmokeVolume::raymarch_rgba / raymarch_projection_rgba (reference src/smoke/render.rs:7-178, bound to
 * Python as SmokeDomain.render_rgba / render_projection_rgba, src/smoke/py.rs:531-625).  Fields are the reference's
 * (x fastest, then y, then z: index = (z * ny + y) * nx + x, types.rs:359-361). */
typedef struct f3d_smoke_volume {
    const float *density, *temperature, *soot, *humidity, *emission, *age; /* emission = emission_rate, age = particle_age */
    uint32_t dims[3];    /* nx, ny, nz (each >= 2; nx*ny*nz <= 256^3 like the reference) */
    float voxel_size[3];
    float origin[3];
    uint32_t frame_index; /* jitter seed term (SmokeVolume::frame_index as u32) */
} f3d_smoke_volume;

typedef struct f3d_smoke_view {
    uint32_t width, height;
    int32_t projection;       /* 0: perspective camera (raymarch_rgba); 1: map-aligned parallel projection */
    float camera_pos[3], target[3], up[3], fovy_deg; /* perspective */
    float view_direction[3];  /* projection */
    float sun_direction[3];
} f3d_smoke_view;

typedef struct f3d_smoke_settings { /* SmokeRenderSettings, reference src/smoke/types.rs:227-269 */
    float density_scale, extinction, scattering, absorption, phase_g, step_size;
    uint32_t max_steps;
    int32_t self_shadow;
    uint32_t shadow_steps;
    float shadow_step_size, jitter_strength, exposure;
    float thin_color[3], dense_color[3];
    float soot_absorption, fire_glow;
} f3d_smoke_settings;

/* rgba: caller-owned height x width x 4 bytes (straight colour, alpha = 1 - transmittance).  kernel_seconds
 * (optional) receives the ray-march kernel's device time.  Errors carry the reference's message texts.
 * Each of the six fields, and rgba, may be a DEVICE pointer: such a field is read where it is and a device image is
 * left on the device (a resident smoke sequence: f3d_smoke_step on device fields -> f3d_smoke_render -> f3d_smoke_composite).
 * The three handle-less smoke entry points launch on the NULL stream, return when their kernels have finished (as in ABI 4)
 * and keep their scratch between calls (freed by f3d_device_pool_trim).  A resident sequence uses the handle below
 * (f3d_smoke_seq_*: own streams, asynchronous calls, scratch freed with the handle).  ABI-5 shim, for one revision: a
 * thread that has called f3d_smoke_set_stream gets round 5's behaviour for its handle-less calls -- they launch on the
 * stream it named and, when their results stay on the device and no time is asked for, return with their launches enqueued. */
int f3d_smoke_render(const f3d_smoke_volume *volume, const f3d_smoke_view *view, const f3d_smoke_settings *settings,
                     uint8_t *rgba, double *kernel_seconds, char *err, size_t errlen);
/* ABI-5 SHIM (superseded by f3d_smoke_seq_*; kept for one revision).
 * The stream (a hipStream_t; NULL = the null stream) on which the calling thread's next f3d_smoke_step / f3d_smoke_render /
 * f3d_smoke_composite calls enqueue.  With the solver on one stream and the marcher on another, step f + 1 runs beside
 * the march of frame f: the marcher reads the volume's fields only in its first kernels (it re-packs them), and
 * f3d_smoke_wait_fields_read makes `stream` wait for exactly that point of the calling thread's LAST f3d_smoke_render
 * (a no-op before the first).  Scratch is per entry point, not per stream: keep each entry point on one stream.
 * (No counterpart in the reference, whose solver and marcher are host loops.) */
void f3d_smoke_set_stream(void *stream);
int f3d_smoke_wait_fields_read(void *stream);

/* ---- smoke transport solver (the 120-frame sequence of BASELINE.json configs[4] needs its fields from somewhere) -----------
 * Replaces SmokeVolume::step / add_emitter (reference src/smoke/sim.rs:7-139, bound to Python as SmokeDomain.step,
 * src/smoke/py.rs:459-480; single-threaded host code there): `steps` steps of the solver on the device -- emitters,
 * forces (wind, buoyancy, procedural turbulence), semi-Lagrangian / MacCormack advection, diffusion, vorticity
 * confinement, Jacobi pressure projection, boundary damping, sub-grid density eddies, decay and ageing.  All fields are
 * caller-owned arrays, read and written in place ((nz, ny, nx) f32, velocity (nz, ny, nx, 3)): nine HOST arrays (uploaded and
 * read back by the call) or nine DEVICE arrays (the solver works on them where they are: nothing crosses the bus). */
typedef struct f3d_smoke_state {
    float *density, *temperature, *fuel, *soot, *humidity, *emission_rate, *particle_age, *velocity, *pressure;
    uint32_t dims[3];
    float voxel_size[3], origin[3];
    float sparse_threshold; /* SmokeDomainConfig::sparse_threshold (default 1e-5) */
    float time_seconds;     /* in/out */
    uint32_t frame_index;   /* in/out */
} f3d_smoke_state;
typedef struct f3d_smoke_step_settings { /* SmokeStepSettings, reference src/smoke/types.rs:142-180 */
    float dt, density_decay, temperature_decay, velocity_damping, diffusion, buoyancy, vorticity;
    uint32_t pressure_iterations;
    float turbulence_strength;
    uint32_t turbulence_seed;
    int32_t mac_cormack, mass_conservation, terrain_collision;
    float boundary_damping;
    float wind[3];
} f3d_smoke_step_settings;
typedef struct f3d_smoke_emitter { /* SmokeEmitter, reference src/smoke/types.rs:69-99 */
    float center[3], radius, density_rate, temperature_rate, fuel_rate, soot_rate, humidity_rate, emission_rate, velocity[3], start_time,
        end_time;
} f3d_smoke_emitter;
int f3d_smoke_step(f3d_smoke_state *state, const f3d_smoke_step_settings *settings, const f3d_smoke_emitter *emitters,
                   uint32_t emitter_count, uint32_t steps, double *device_seconds, char *err, size_t errlen);

/* ---- smoke over terrain: the per-pixel composites of BASELINE.json configs[4] ----
 * The reference builds each frame of its smoke sequence on the host with numpy and Pillow
 * (examples/california_cigar_smoke_demo.py, tested by tests/test_california_cigar_smoke_hybrid.py);
 * these are the same three operations as one device pass over RGBA8 images:
 *   F3D_COMPOSITE_ATMOSPHERIC  composite_atmospheric_smoke(base, layer)   :8527-8544 -- a ray-marched smoke layer
 *                              (f3d_smoke_render) over a path-traced terrain frame; the output alpha is 255
 *   F3D_COMPOSITE_SMOKE_MAPS   composite_main_smoke_maps(base = atmospheric, layer = physical or NULL,
 *                              base_alpha, layer_alpha) :3367-3380, alpha capped at max_alpha
 *   F3D_COMPOSITE_OVER         PIL.Image.alpha_composite(base, layer placed at offset) (:8721-8725, :3335-3349);
 *                              the layer may have its own size and is clipped to the base
 * base, layer and out may be host or device pointers (width * height * 4 bytes, rows tightly packed); out may
 * alias base.  kernel_seconds (may be NULL) receives the device time of the pass. */
#define F3D_COMPOSITE_ATMOSPHERIC 0u
#define F3D_COMPOSITE_SMOKE_MAPS 1u
#define F3D_COMPOSITE_OVER 2u
typedef struct f3d_composite_desc {
    uint32_t struct_size; /* sizeof(f3d_composite_desc) of the caller's header */
    uint32_t mode;
    uint32_t width, height;             /* base and output */
    uint32_t layer_width, layer_height; /* must equal width, height except in F3D_COMPOSITE_OVER */
    int32_t offset_x, offset_y;         /* F3D_COMPOSITE_OVER only, else 0 */
    const uint8_t *base;
    const uint8_t *layer; /* NULL only in F3D_COMPOSITE_SMOKE_MAPS (`physical_rgba is None`) */
    float base_alpha, layer_alpha; /* F3D_COMPOSITE_SMOKE_MAPS: atmospheric_alpha (0.42), physical_alpha (0.92) */
    uint32_t max_alpha;            /* F3D_COMPOSITE_SMOKE_MAPS: HYBRID_SMOKE_MAX_ALPHA (168) */
} f3d_composite_desc;
int f3d_smoke_composite(const f3d_composite_desc *desc, uint8_t *out_rgba, double *kernel_seconds, char *err, size_t errlen);

/* ---- a resident smoke sequence behind a handle (ABI 6) ----
 * BASELINE.json configs[4] is a 120-frame sequence: per frame a solver step, a march, a composite, all on state that stays
 * on the device.  The handle holds what such a sequence needs between calls -- which stream the solver runs on and which the
 * marcher (the caller's hipStream_t values, which must outlive the handle; NULL = the null stream; the same stream twice =
 * no overlap), the order between them, and the scratch of the three entry points:
 *   f3d_smoke_seq_step       runs on the solver's stream, behind the last render's READS of the fields (the marcher re-packs
 *                            the fields in its first kernels; the rest of the march runs beside the next step);
 *   f3d_smoke_seq_render     runs on the marcher's stream, behind the last step;
 *   f3d_smoke_seq_composite  runs on the marcher's stream (behind the render whose layer it reads).
 * Arguments are those of f3d_smoke_step / f3d_smoke_render / f3d_smoke_composite.  A call whose results stay on the device
 * and whose time pointer is NULL returns with its launches enqueued: order other streams behind the handle's streams
 * (f3d_smoke_seq_streams + an event) before reading its outputs; kernel errors then surface in a later call.
 * f3d_smoke_seq_destroy waits for both streams and gives the sequence's scratch back.  Two handles share nothing; one
 * handle is for one thread at a time.  The reference has no counterpart (its solver and marcher are single-threaded host
 * loops, src/smoke/sim.rs:270-317, src/smoke/render.rs:7-96). */
typedef struct f3d_smoke_seq f3d_smoke_seq;
typedef struct f3d_smoke_seq_stats_t {
    uint64_t scratch_bytes;               /* device memory the sequence holds between calls */
    uint32_t shadow_list_chunks;          /* capacity of the marcher's deferred self-shadow list in the last render, in chunks */
    uint32_t shadow_list_chunks_used;     /* chunks that render asked for (above the capacity: the excess was walked in the one-kernel form) */
    uint32_t shadow_list_slots_per_chunk; /* 52 bytes a slot */
    uint32_t reserved;
} f3d_smoke_seq_stats_t;
int f3d_smoke_seq_create(void *stream_solver, void *stream_march, f3d_smoke_seq **out, char *err, size_t errlen);
void f3d_smoke_seq_destroy(f3d_smoke_seq *seq);
int f3d_smoke_seq_streams(f3d_smoke_seq *seq, void **stream_solver, void **stream_march);
int f3d_smoke_seq_step(f3d_smoke_seq *seq, f3d_smoke_state *state, const f3d_smoke_step_settings *settings, const f3d_smoke_emitter *emitters,
                       uint32_t emitter_count, uint32_t steps, double *device_seconds, char *err, size_t errlen);
int f3d_smoke_seq_render(f3d_smoke_seq *seq, const f3d_smoke_volume *volume, const f3d_smoke_view *view, const f3d_smoke_settings *settings,
                         uint8_t *rgba, double *kernel_seconds, char *err, size_t errlen);
int f3d_smoke_seq_composite(f3d_smoke_seq *seq, const f3d_composite_desc *desc, uint8_t *out_rgba, double *kernel_seconds, char *err, size_t errlen);
/* What the sequence holds and the fill of its last render's self-shadow list (waits for that render).  After
 * f3d_device_pool_trim, which frees the scratch of live sequences too, it reports scratch_bytes = 0 until the next step
 * or render, and no list (shadow_list_chunks = shadow_list_chunks_used = 0) until the next render. */
int f3d_smoke_seq_stats(f3d_smoke_seq *seq, f3d_smoke_seq_stats_t *out, char *err, size_t errlen);

/* ---- AETHER acceptance reference: stochastic spectral transport (no LUT, black environment) ----
 * Replaces _forge3d.hybrid_render_aether_spectral_reference (reference src/py_functions/path_tracing/
 * aether_reference.rs:14-146 -> HybridPathTracer::render_aether_spectral_reference, hybrid_compute/
 * aether_reference.rs:203-560 -> WGSL main_aether_spectral_reference, shaders/atmosphere/
 * prometheus_spectral_reference.wgsl:423-480): delta-tracking paths at 11 wavelengths over the terrain tracer's own
 * camera rays, heightfield hits and sun visibility; the acceptance check of the LUT post pass (f3d_terrain_ref_desc.
 * atmosphere).  Same validation and messages as the reference (status F3D_STATUS_RENDER), plus: the DEM must lie
 * inside the top of the atmosphere (a terrain hit then always precedes the top-of-atmosphere exit, which the
 * reference's shadow test assumes).  At most 8 000 000 wavelength paths (width * height * spp * 11). */
typedef struct f3d_aether_ref_desc { /* AetherSpectralReferenceDesc, aether_reference.rs:14-43 */
    uint32_t struct_size;            /* sizeof(f3d_aether_ref_desc) of the caller's header */
    uint32_t dem_width, dem_height;
    const float *heights;            /* row-major (dem_height, dem_width) */
    float spacing_x, spacing_z, exaggeration;
    float cam_origin[3], cam_look_at[3], cam_up[3], fov_y_deg;
    float sun_azimuth_deg, sun_elevation_deg, sun_intensity;
    float turbidity, ozone_du, mie_g, ground_albedo;
    uint32_t width, height, seed, spp;
    int32_t enabled;                 /* 0: explicit black (all outputs zero, converged) */
    float variance_threshold;
} f3d_aether_ref_desc;
typedef struct f3d_aether_ref_out { /* AetherSpectralReferenceOutput, aether_reference.rs:46-60 */
    float *mean_xyz;   /* width * height * 3: unclipped per-pixel mean CIE XYZ */
    float *linear_rgb; /* width * height * 3: max(signed linear RGB of the mean, 0) */
    float variance;    /* max over pixels of the estimated variance of the sample-mean CIE Y */
    int32_t converged;
    uint64_t terrain_primary_hits; /* camera samples whose primary ray hit the terrain */
    uint64_t gpu_resource_bytes;
    double kernel_seconds;         /* device time of the three launches */
} f3d_aether_ref_out;
int f3d_aether_reference_render(const f3d_aether_ref_desc *desc, f3d_aether_ref_out *out, char *err, size_t errlen);

/* ---- test hooks (KATs restated from the reference's Rust unit tests) ----------- */
/* build_minmax_mips on the GPU (reference terrain_heightfield.rs:132-202); output in
 * the reference's layout: levels back to back, finest first, each (ph, pw, 2) f32;
 * dims_out (pw, ph) pairs.  levels_out may be NULL to query level count / size. */
int f3d_build_minmax_mips(const float *heights, uint32_t width, uint32_t height, float *levels_out,
                          uint32_t *dims_out, uint32_t max_levels, uint64_t *total_floats, char *err,
                          size_t errlen);
/* terrain_trace over a ray batch (reference test seam
 * main_helios_production_terrain_trace_proof, terrain_heightfield.rs:1646-1671).
 * rays: n x 8 f32 (origin xyz, tmin, direction xyz, tmax). */
int f3d_terrain_trace_batch(const float *heights, uint32_t width, uint32_t height, float origin_x,
                            float origin_z, float spacing_x, float spacing_z, float exaggeration,
                            float inv_two_r_prime, uint32_t curvature_enabled, const float *rays,
                            uint32_t n, int32_t any_hit, int32_t apply_curvature, uint32_t *out_hit,
                            float *out_t, float *out_normal, char *err, size_t errlen);
/* geo::refraction::effective_radius_m (reference src/geo/refraction.rs:137-148). */
int f3d_effective_radius_m(int32_t earth_model, double latitude_deg, double sphere_radius_m,
                           int32_t refraction_model, double pressure_mbar, double temperature_c,
                           double refraction_k, double azimuth_deg, double *radius_out, char *err,
                           size_t errlen);

/* Scene cache: the acceleration tables of the most recently rendered DEMs (default 2 per process) stay on the
 * device and are shared by every session / one-shot call that renders the same heights, dims and exaggeration --
 * a camera path does not rebuild them per frame.  0 entries switches the cache off and frees it. */
void f3d_scene_cache_limit(uint32_t entries);
uint32_t f3d_scene_cache_entries(void);

int f3d_device_count(void);
const char *f3d_device_name(int32_t device); /* gcnArchName, "" when unavailable */
const char *f3d_version(void);
/* F3D_ABI_VERSION the library was built with: a binding checks it once after loading. */
uint32_t f3d_abi_version(void);
/* First 16 hex digits of the SHA-256 of the sources + compiler flags the library was built from ("unknown" for a
 * build that did not go through __graft_entry__.build_hip). */
const char *f3d_source_digest(void);
/* Diagnostics (f3d_devmem.h): pattern 0..255 = every device buffer the library allocates from now on lies between two
 * 256 KiB guard regions and buffer and guards are filled with that byte; negative = off.  No result may depend on the
 * pattern: a dependence means a kernel reads memory nobody wrote (uninitialised, or beyond a buffer).  The environment
 * variable F3D_POISON=<0..255> starts a process in this mode. */
void f3d_debug_poison(int32_t pattern);

#ifdef __cplusplus
}
#endif
#endif /* F3D_TERRAIN_PT_H */
