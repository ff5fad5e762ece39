// f3d_host_update.h -- part of f3d_host.hip (included there once, after the session's enqueue helpers): the updates of a live
// session -- re-arm (sun / seed / exposure / IBL intensity / frame budget), re-aim (+ camera), re-mesh (+ a moved or another
// mesh), re-terrain (+ new DEM samples) -- and their C ABI: what they share in Update, what is an update's own in its function.
// Behind them what every later entry of a live session uses too (queries, rasters, drape): check_budget, grow_scratch,
// check_flags, check_no_wait, update_entry.
#pragma once

namespace {

// A new render on a live session: the descriptor's re-armable members replaced (and, aim given, the camera), validated and
// turned into uniforms by the create's own code, then k_rearm -- or, for a new camera, k_reaim -- on the session stream behind
// everything enqueued so far.  An update is: Update u(...) [the clock, the struct sizes of aim and its arm, the peer-halo
// refusal, the descriptor with the new members], its own checks on u.d, u.validate() [validate_desc, fill_uniforms], its own
// device step, u.apply() [uniforms, pass, host state].  Every refusal comes before the first change of the session.  A
// re-arm or re-aim allocates nothing and waits for nothing.
struct Update {
    f3d_session &s;
    const bool cam;
    const double t_host = now_s();
    f3d_terrain_ref_desc d;
    FrameParams U{};
    bool require_valid = false;

    Update(f3d_session &session, const f3d_session_rearm_desc &r, const f3d_session_reaim_desc *aim, const char *done)
        : s(session), cam(aim != nullptr) {
        if (aim) check_struct_size(*aim, "f3d_session_reaim_desc");
        check_struct_size(r, "f3d_session_rearm_desc");
        if (s.peer[0].connected || s.peer[1].connected)
            fail(F3D_STATUS_VALUE, "a session with peer halos cannot be %s: the frame counters its neighbours poll only rise", done);
        d = s.desc;
        d.sun_azimuth_deg = r.sun_azimuth_deg;
        d.sun_elevation_deg = r.sun_elevation_deg;
        d.sun_intensity = r.sun_intensity;
        for (int c = 0; c < 3; c++) d.sun_color[c] = r.sun_color[c];
        d.exposure = r.exposure;
        d.env_intensity = r.env_intensity;
        d.seed = r.seed;
        d.max_frames = r.max_frames;
        d.min_frames = r.min_frames;
        d.variance_threshold = r.variance_threshold;
        d.observer_latitude_deg = r.observer_latitude_deg;
        d.observer_longitude_deg = r.observer_longitude_deg;
        d.pressure_mbar = r.pressure_mbar;
        d.temperature_c = r.temperature_c;
        if (aim) {
            for (int c = 0; c < 3; c++) {
                d.cam_origin[c] = aim->cam_origin[c];
                d.cam_look_at[c] = aim->cam_look_at[c];
                d.cam_up[c] = aim->cam_up[c];
            }
            d.fov_y_deg = aim->fov_y_deg;
        }
    }

    // own_scan: a check of the update's own that looks at every value of its payload.  It sits behind validate_desc's cheap
    // checks and in front of fill_uniforms, which refuses too (observer latitude / longitude, the earth and refraction
    // models): re-terrain's non-finite scan has always won over those, and the order in which refusals win is contract.
    template <class Scan>
    void validate(Scan &&own_scan) {
        validate_desc(d);
        own_scan();
        require_valid = fill_uniforms(d, U);
    }
    void validate() { validate([] {}); }

    void apply() {
        // (DEM transform, spacing and spp are the create's, and without a re-aim the camera: fill_uniforms gives them the same
        // bits again.  The AETHER post reads the camera from these uniforms at resolve time: its record holds no camera term.)
        FrameParams &P = s.params;
        P.cam = U.cam;
        P.light = U.light;
        P.terrain.inv_two_r_prime = U.terrain.inv_two_r_prime;
        P.terrain.curvature_enabled = U.terrain.curvature_enabled;
        P.env.intensity = U.env.intensity;
        P.same_sun = same_sun_of(P);
        if (s.aether.enabled) aether_sun_terms(s.aether, d);
        s.require_valid_reservoirs = require_valid;
        s.desc = d;
        s.desc.mesh_vertices = nullptr;  // (a re-mesh validated them through d: read during the call only)
        s.desc.mesh_indices = nullptr;

        join_bands(s);  // (the session stream after every band launch so far: the clears follow the last frame's kernels)
        P.band_begin = s.row_begin;
        P.band_end = s.row_end;
        P.frame_index = 0;
        P.trace_first = 0u;
        P.res_in = s.res[1];
        P.res_out = s.res[0];
        P.collect_stats = 0;
        P.tile_order = nullptr;
        P.tile_cost = nullptr;
        RearmParams R{};
        R.frame = P;
        R.gbuffer_n = s.gbuffer_n;
        R.depth = s.depth;
        R.res[0] = s.res[0];
        R.res[1] = s.res[1];
        R.tile_cost = s.tile_cost;
        R.tiles = s.tile_cost ? frame_tile_count(P, nullptr) : 0u;
        if (cam) {
            hip_check(launch_reaim(R, s.stream), "re-aim kernel");
            enqueue_sky_blocks(s);  // (new primary-ray certificates: the deep-sky table of the new view, f3d_skyblocks.h)
        } else {
            hip_check(launch_rearm(R, s.stream), "re-arm kernel");
        }
        // host-side frame state as a new session has it
        s.cost_frame = s.order_frame = -1;
        s.rendered = false;
        s.trace_first = -1;
        s.trace_count = 0;
        for (auto &b : s.bands) {
            b.last = -1;
            b.unjoined = false;
        }
        s.reaim_seconds = cam ? now_s() - t_host : 0.0;
    }
};

// An update that allocates: the tracked total it plans (the shared entry's bytes dropped, its own added) against the budget.
void check_budget(const f3d_session &s, uint64_t planned, const char *update, const char *brings) {
    if (planned > s.budget)
        fail(F3D_STATUS_RENDER, "%s exceeds the memory budget: %s the tracked total to %llu > limit %llu", update, brings,
             (unsigned long long)planned, (unsigned long long)s.budget);
}

// A scratch of the session that only grows (the query's, the rasters'): for a call that wants more than it holds, the larger
// buffer is taken and committed, then the old one goes back -- nothing is in flight on it for the blocking host forms; a paint
// (f3d_host_paint.h) returns with kernels enqueued on its buffers and relies on Ledger::free waiting for the device.
void grow_scratch(f3d_session &s, void *&scratch, uint64_t &bytes, uint64_t want, const char *noun, const char *brings, const char *what) {
    if (want <= bytes) return;
    check_budget(s, s.mem.device_bytes - bytes + want, noun, brings);
    Ledger::Take take{s.mem};
    void *fresh = take((size_t)want, what);
    take.commit();
    if (scratch) s.mem.free(scratch, (size_t)bytes);
    scratch = fresh;
    bytes = want;
}

// The flags every entry with a host and a device form shares, under the values of all their families (f3d_terrain_pt.h).
constexpr uint32_t kDevicePointers = 4u, kNoWait = 8u;
static_assert(F3D_QUERY_DEVICE_POINTERS == kDevicePointers && F3D_RASTER_DEVICE_POINTERS == kDevicePointers && F3D_HORIZON_DEVICE_POINTERS == kDevicePointers &&
              F3D_IRRADIATION_DEVICE_POINTERS == kDevicePointers && F3D_CLEARANCE_DEVICE_POINTERS == kDevicePointers && F3D_DRAPE_DEVICE_POINTERS == kDevicePointers &&
              F3D_QUERY_NO_WAIT == kNoWait && F3D_RASTER_NO_WAIT == kNoWait && F3D_HORIZON_NO_WAIT == kNoWait && F3D_IRRADIATION_NO_WAIT == kNoWait &&
              F3D_CLEARANCE_NO_WAIT == kNoWait && F3D_DRAPE_NO_WAIT == kNoWait, "one DEVICE_POINTERS and one NO_WAIT for every family");

void check_flags(uint32_t flags, uint32_t known, const char *noun, const char *names) {
    if (flags & ~known) fail(F3D_STATUS_VALUE, "unknown %s flags 0x%x (%s)", noun, flags, names);
}

// Returns whether the call is in the device form; `why`: what the host form promises at its return.
bool check_no_wait(uint32_t flags, const char *why = "results in host memory are there") {
    const bool device_form = (flags & kDevicePointers) != 0u;
    if ((flags & kNoWait) && !device_form) fail(F3D_STATUS_VALUE, "NO_WAIT needs DEVICE_POINTERS: %s when the call returns", why);
    return device_form;
}

void rearm(f3d_session &s, const f3d_session_rearm_desc &r) {
    Update u(s, r, nullptr, "re-armed");
    u.validate();
    u.apply();
}

void reaim(f3d_session &s, const f3d_session_reaim_desc &a) {
    Update u(s, a.arm, &a, "re-aimed");
    u.validate();
    u.apply();
}

// ---- re-mesh: the mesh of a live session moved (refit) or replaced (the create's path), then a re-aim ------------------
// Positions only: the session's own copy of vertices, leaf-order triangles and nodes (made at the first refit; the cache
// entry other sessions share is never written), the vertex upload in stream order, then the refit passes of
// f3d_bvh_refit.h -- all on the session stream behind everything enqueued so far, no wait for the device.
void remesh_refit(f3d_session &s, const float *vertices, uint32_t vertex_count) {
    FrameParams &P = s.params;
    f3d_session::OwnMesh &O = s.own_mesh;
    const CachedMesh &E = *s.mesh;
    const bool first = !O.live;
    const uint32_t nodes = E.dev.bvh4_nodes ? E.dev.bvh4_node_count : E.dev.bvh_node_count;
    if (first) {
        f3d_session::OwnMesh N;
        N.vertex_bytes = E.vertex_bytes;
        N.tri_bytes = E.tri_bytes;
        N.node_bytes = E.node_bytes;
        N.link_bytes = (size_t)std::max(nodes, 1u) * sizeof(uint32_t);
        N.bounds_bytes = 12u * sizeof(int);
        // (the indices stay the entry's)
        check_budget(s, s.mem.device_bytes - s.mesh_counted + E.index_bytes + N.bytes(), "re-mesh",
                     "the session's own copy of the mesh and the refit tables bring");
        Ledger::Take take{s.mem};
        N.vertices = (float4 *)take(N.vertex_bytes, "re-mesh vertices");
        if (N.tri_bytes) N.tris = (float4 *)take(N.tri_bytes, "re-mesh BVH triangles");
        if (N.node_bytes) N.nodes = take(N.node_bytes, "re-mesh BVH nodes");
        N.parent = (uint32_t *)take(N.link_bytes, "re-mesh parent links");
        N.counter = (uint32_t *)take(N.link_bytes, "re-mesh arrival counters");
        N.bounds = (int *)take(N.bounds_bytes, "re-mesh scene bounds");
        take.commit();
        s.mem.device_bytes -= s.mesh_counted;
        s.mesh_counted = E.index_bytes;
        s.mem.device_bytes += s.mesh_counted;
        join_bands(s);
        // topology words and the triangles' index words from the shared entry; counters at zero; both bound sets empty
        if (N.tris) hip_check(hipMemcpyAsync(N.tris, E.dev.bvh_tris, N.tri_bytes, hipMemcpyDeviceToDevice, s.stream), "re-mesh copy");
        if (N.nodes)
            hip_check(hipMemcpyAsync(N.nodes, E.dev.bvh4_nodes ? (const void *)E.dev.bvh4_nodes : (const void *)E.dev.bvh_nodes, N.node_bytes,
                                     hipMemcpyDeviceToDevice, s.stream), "re-mesh copy");
        hip_check(hipMemsetAsync(N.counter, 0, N.link_bytes, s.stream), "re-mesh counters");
        static const int kEmptyBounds[12] = {0x7F800000, 0x7F800000, 0x7F800000, (int)0x807FFFFF, (int)0x807FFFFF, (int)0x807FFFFF,
                                             0x7F800000, 0x7F800000, 0x7F800000, (int)0x807FFFFF, (int)0x807FFFFF, (int)0x807FFFFF};
        hip_check(hipMemcpyAsync(N.bounds, kEmptyBounds, sizeof(kEmptyBounds), hipMemcpyHostToDevice, s.stream), "re-mesh bounds");
        N.live = true;
        O = N;
        P.mesh.vertices = O.vertices;
        if (O.tris) P.mesh.bvh_tris = O.tris;
        if (O.nodes && E.dev.bvh4_nodes) P.mesh.bvh4_nodes = (const Bvh4Node *)O.nodes;
        else if (O.nodes) P.mesh.bvh_nodes = (const BvhNode *)O.nodes;
    } else {
        join_bands(s);
    }
    const std::vector<float> v4 = pad_rgb_to_rgba(vertices, vertex_count, 0.0f);
    upload_staged(O.vertices, v4.data(), v4.size() * sizeof(float), s.stream, true);
    RefitParams R{};
    R.vertices = O.vertices;
    R.indices = E.dev.indices;
    R.tris = O.tris;
    R.tri_count = O.tris ? E.index_count / 3u : 0u;
    if (E.dev.bvh4_nodes) {
        R.wide = (Bvh4Node *)O.nodes;
        R.wide_count = nodes;
    } else {
        R.nodes = (BvhNode *)O.nodes;
        R.node_count = nodes;
    }
    R.parent = O.parent;
    R.counter = O.counter;
    R.bounds = O.bounds + 6u * (O.refits & 1u);
    R.bounds_next = O.bounds + 6u * ((O.refits & 1u) ^ 1u);
    hip_check(launch_bvh_refit(R, first, s.stream), "BVH refit kernels");
    O.refits++;
}

// Another mesh: the create's path with the session's builder (cache, host SAH or LBVH; may wait and allocate like a create).
void remesh_replace(f3d_session &s, const f3d_terrain_ref_desc &d) {
    std::shared_ptr<CachedMesh> fresh = acquire_mesh(s.device, d.mesh_vertices, d.mesh_vertex_count, d.mesh_indices, d.mesh_index_count,
                                                     s.mesh_builder, s.stream);
    check_budget(s, s.mem.device_bytes - s.mesh_counted - s.own_mesh.bytes() + fresh->mem.device_bytes, "re-mesh", "the new mesh brings");
    // the old mesh goes only after the work enqueued before this call has finished
    join_bands(s);
    hip_check(hipStreamSynchronize(s.stream), "re-mesh");
    s.own_mesh.release(s.mem);
    s.mem.device_bytes -= s.mesh_counted;
    s.mesh = fresh;
    s.mesh_counted = fresh->mem.device_bytes;
    s.mem.device_bytes += s.mesh_counted;
    s.params.mesh = fresh->dev;
}

void remesh(f3d_session &s, const f3d_session_remesh_desc &m) {
    check_struct_size(m, "f3d_session_remesh_desc");
    Update u(s, m.aim.arm, &m.aim, "re-meshed");
    if (!s.mesh)
        fail(F3D_STATUS_VALUE, "this session was created without a mesh: a re-mesh moves or replaces a session's mesh, it cannot give it one");
    if (s.mesh_grid)
        fail(F3D_STATUS_VALUE, "this session's occlusion rays march a mesh grid made from the create's mesh (F3D_MESH_FUSED build): it cannot be re-meshed");
    if (m.mesh_indices) {  // another mesh: every mesh check of the create
        u.d.mesh_vertices = m.mesh_vertices;
        u.d.mesh_vertex_count = m.mesh_vertex_count;
        u.d.mesh_indices = m.mesh_indices;
        u.d.mesh_index_count = m.mesh_index_count;
    } else {  // positions only: the create's vertex checks, with its texts and statuses (validate_desc, f3d_setup.h)
        if (!m.mesh_vertices || m.mesh_vertex_count == 0) fail(F3D_STATUS_RENDER, "mesh vertices must be a non-empty flat [x,y,z] list");
        if (m.mesh_vertex_count != s.params.mesh.vertex_count)
            fail(F3D_STATUS_VALUE, "a re-mesh without mesh_indices moves the session's mesh: %u vertices given, its topology has %u (pass "
                 "mesh_indices for another mesh)", m.mesh_vertex_count, s.params.mesh.vertex_count);
        for (size_t i = 0; i < (size_t)m.mesh_vertex_count * 3; i++)
            if (!std::isfinite(m.mesh_vertices[i])) fail(F3D_STATUS_RENDER, "mesh vertices contain non-finite values");
    }
    u.validate();
    if (m.mesh_indices) remesh_replace(s, u.d);
    else remesh_refit(s, m.mesh_vertices, m.mesh_vertex_count);
    u.apply();
}

// ---- re-terrain: new DEM samples on a live session, its tables patched on the GPU, then a re-aim -------------------------
// The block is uploaded in stream order into the session's staging buffer and the two passes of f3d_retable.h patch the
// session's OWN leaf and band tables (taken at the first call and filled from the shared scene-cache entry by device
// copies; that entry is never written and stays referenced -- the copies read it -- but is no longer counted).  All on the
// session stream behind everything enqueued so far, no wait for the device; only the first call, and a call with a block
// larger than any before (the staging buffer grows: the old one goes back through the allocator, which waits for the work
// that reads it), allocate.
void reterrain(f3d_session &s, const f3d_session_reterrain_desc &t) {
    check_struct_size(t, "f3d_session_reterrain_desc");
    Update u(s, t.aim.arm, &t.aim, "re-terrained");
    if (s.mesh_grid)
        fail(F3D_STATUS_VALUE, "this session's occlusion rays march a mesh grid binned on the create's terrain cells (F3D_MESH_FUSED build): it cannot be re-terrained");
    if (s.params.terrain.horizon)
        fail(F3D_STATUS_VALUE, "this session built the far-horizon table of its DEM (F3D_IBL_HORIZON=1): it cannot be re-terrained, the table would be stale");
    const uint32_t w = s.desc.dem_width, h = s.desc.dem_height;
    if (!t.heights || t.width == 0u || t.height == 0u)
        fail(F3D_STATUS_VALUE, "re-terrain block is empty (%ux%u samples): a block holds at least one sample", t.width, t.height);
    if (t.x0 >= w || t.y0 >= h || t.width > w - t.x0 || t.height > h - t.y0)
        fail(F3D_STATUS_VALUE, "re-terrain block of %ux%u samples at sample (%u, %u) leaves the session's %ux%u DEM (another DEM size needs a new session)",
             t.width, t.height, t.x0, t.y0, w, h);
    const bool whole = t.x0 == 0u && t.y0 == 0u && t.width == w && t.height == h;
    if (t.exaggeration != 0.0f && !(t.exaggeration == s.desc.exaggeration)) {
        if (!whole)
            fail(F3D_STATUS_VALUE, "a new exaggeration (%g, the session's is %g) rescales every sample: give it with the whole %ux%u DEM, not with a block",
                 (double)t.exaggeration, (double)s.desc.exaggeration, w, h);
        u.d.exaggeration = t.exaggeration;
    }
    const size_t samples = (size_t)t.width * t.height, block_bytes = samples * sizeof(float);
    u.validate([&] {
        uint32_t bad = 0u;  // (an exponent field of all ones: inf / NaN)
        for (size_t i = 0; i < samples; i++) {
            uint32_t v;
            memcpy(&v, t.heights + i, sizeof v);
            bad |= (uint32_t)((v & 0x7F800000u) == 0x7F800000u);
        }
        if (bad) fail(F3D_STATUS_UPLOAD, "terrain heightfield contains non-finite samples");
    });

    f3d_session::OwnTerrain &O = s.own_terrain;
    const TableLayout &L = s.tables.layout;
    const size_t leaf_bytes = L.leaf_count * sizeof(LeafRec), band_bytes = L.band_count * sizeof(NodeRec);
    const bool take_tables = !O.leaves, grow = block_bytes > O.staging_bytes;
    if (take_tables || grow) {
        char brings[96];
        snprintf(brings, sizeof brings, "the session's own tables and the staging buffer of a %ux%u block bring", t.width, t.height);
        check_budget(s, s.mem.device_bytes - (take_tables ? s.scene_counted : 0u) + (take_tables ? leaf_bytes + band_bytes : 0u) -
                            (grow ? O.staging_bytes : 0u) + (grow ? block_bytes : 0u), "re-terrain", brings);
        f3d_session::OwnTerrain N = O;
        Ledger::Take take{s.mem};
        if (grow) {
            N.staging = (float *)take(block_bytes, "re-terrain staging");
            N.staging_bytes = block_bytes;
        }
        if (take_tables) {
            N.leaves = (LeafRec *)take(leaf_bytes, "re-terrain leaf table");
            N.bands = (NodeRec *)take(band_bytes, "re-terrain band tables");
            N.leaf_bytes = leaf_bytes;
            N.band_bytes = band_bytes;
        }
        take.commit();
        if (grow && O.staging) s.mem.free(O.staging, O.staging_bytes);
        if (take_tables) {
            s.mem.device_bytes -= s.scene_counted;
            s.scene_counted = 0u;
        }
        O = N;
    }
    join_bands(s);
    if (!O.live) {
        hip_check(hipMemcpyAsync(O.leaves, s.tables.leaves, leaf_bytes, hipMemcpyDeviceToDevice, s.stream), "re-terrain copy");
        hip_check(hipMemcpyAsync(O.bands, s.tables.bands, band_bytes, hipMemcpyDeviceToDevice, s.stream), "re-terrain copy");
    }
    upload_staged(O.staging, t.heights, block_bytes, s.stream, true);
    hip_check(launch_retable(retable_params(L, O.staging, t.x0, t.y0, t.width, t.height, u.d.exaggeration, O.leaves, O.bands), s.stream),
              "re-terrain table kernels");
    if (!O.live) {
        O.live = true;
        s.tables.leaves = O.leaves;
        s.tables.bands = O.bands;
        s.tables.dev.leaves = O.leaves;
        s.tables.dev.bands = O.bands;
        s.params.terrain.leaves = O.leaves;
        s.params.terrain.bands = O.bands;
        s.params.terrain.mesh_bands = O.bands;  // (no mesh grid: refused above)
    }
    u.apply();
}

// The door of an update behind the C ABI: the session's device bound, a descriptor that is there.
template <class Desc>
int update_entry(f3d_session *s, const Desc *desc, const char *noun, void (*update)(f3d_session &, const Desc &), char *err, size_t errlen) {
    return c_abi(err, errlen, [&] {
        DeviceGuard g(checked(s).device);
        if (!desc) fail(F3D_STATUS_VALUE, "null %s descriptor", noun);
        update(*s, *desc);
    });
}

}  // namespace

extern "C" {

int f3d_session_rearm(f3d_session *s, const f3d_session_rearm_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "re-arm", rearm, err, errlen);
}

int f3d_session_reaim(f3d_session *s, const f3d_session_reaim_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "re-aim", reaim, err, errlen);
}

int f3d_session_remesh(f3d_session *s, const f3d_session_remesh_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "re-mesh", remesh, err, errlen);
}

int f3d_session_reterrain(f3d_session *s, const f3d_session_reterrain_desc *desc, char *err, size_t errlen) {
    return update_entry(s, desc, "re-terrain", reterrain, err, errlen);
}

}  // extern "C"
