// tests/emul/host_scene.h -- TEST INFRASTRUCTURE ONLY (the host harnesses include it after ../emul/f3d_emul.cpp).
// The scene of a descriptor as the emulator's render sets it up: the product's uniforms, host-built tables and mesh BVHs.
#pragma once

namespace {
struct HostScene {
    FrameParams P{};
    HostTables t;
    std::vector<float> mesh4;
    MeshBvh bvh;
    std::vector<Bvh4Node> bvh4;
};

// mesh_form 1 = binary BVH walk, 2 = four wide; rows [row_begin, row_end) of the image (0, 0: all)
void setup(HostScene &S, const f3d_terrain_ref_desc *d, int mesh_form, uint32_t row_begin, uint32_t row_end) {
    validate_desc(*d);
    validate_scene(*d);
    FrameParams &P = S.P;
    (void)fill_uniforms(*d, P);
    S.t = build_tables_host(d->heights, d->dem_width, d->dem_height, d->exaggeration);
    S.t.attach(P.terrain);
    S.t.attach_horizon(P.terrain);
    if (d->mesh_vertices) {
        S.mesh4 = pad_rgb_to_rgba(d->mesh_vertices, d->mesh_vertex_count, 0.0f);
        P.mesh.vertices = (const float4 *)S.mesh4.data();
        P.mesh.indices = d->mesh_indices;
        P.mesh.vertex_count = d->mesh_vertex_count;
        P.mesh.index_count = d->mesh_index_count;
        P.mesh.traversal_mode = 0u;
        S.bvh = build_mesh_bvh(d->mesh_vertices, d->mesh_vertex_count, d->mesh_indices, d->mesh_index_count);
        P.mesh.bvh_nodes = S.bvh.nodes.data();
        P.mesh.bvh_tris = (const float4 *)S.bvh.tris.data();
        P.mesh.bvh_node_count = (uint32_t)S.bvh.nodes.size();
        if (mesh_form == 2) {
            S.bvh4 = collapse_bvh4(S.bvh);
            if (!S.bvh4.empty()) {
                P.mesh.bvh4_nodes = S.bvh4.data();
                P.mesh.bvh4_node_count = (uint32_t)S.bvh4.size();
            }
            S.t.attach_mesh_grid(P.terrain, d->mesh_vertices, d->mesh_vertex_count, d->mesh_indices, d->mesh_index_count);
        }
    }
    P.row_begin = row_begin;
    P.row_end = row_end ? row_end : d->height;
}

// What a harness's *_scene_create exports: the whole image's scene (mesh_form 2: four wide, else the binary walk), null when
// the descriptor is refused.  info (may be null) takes the first info_count of
//     terrain origin x, origin z, spacing x, spacing z, inv_two_r_prime, curvature_enabled, light.wi x, y, z.
HostScene *scene_create(const f3d_terrain_ref_desc *d, int mesh_form, float *info, uint32_t info_count) {
    HostScene *S = new HostScene();
    try {
        setup(*S, d, mesh_form == 2 ? 2 : 1, 0u, 0u);
    } catch (const Failure &) {
        delete S;
        return nullptr;
    }
    const TerrainDev &T = S->P.terrain;
    const float all[9] = {T.origin_x, T.origin_z, T.spacing_x, T.spacing_z, T.inv_two_r_prime, (float)T.curvature_enabled,
                          S->P.light.wi.x, S->P.light.wi.y, S->P.light.wi.z};
    for (uint32_t k = 0; info && k < info_count && k < 9u; k++) info[k] = all[k];
    return S;
}

// a harness-only `origins` / `samples` output: point n of rows * cols x 3 (out may be null)
void store_point(float *out, size_t n, V3 p) {
    if (out) out[3u * n] = p.x, out[3u * n + 1u] = p.y, out[3u * n + 2u] = p.z;
}

// The terrain of the -D*_DRIVER sanitizer programs: a synthetic w x h DEM (its tables in `tables`, which the terrain points
// into), 30 x 25 spacing, centred, curvature enabled.
void driver_terrain(uint32_t w, uint32_t h, HostTables &tables, TerrainDev &T) {
    std::vector<float> dem((size_t)w * h);
    for (uint32_t z = 0; z < h; z++)
        for (uint32_t x = 0; x < w; x++) dem[(size_t)z * w + x] = 3.0f * std::sin(0.37f * (float)x) * std::cos(0.23f * (float)z) + 0.05f * (float)((x * 7u + z * 13u) % 11u);
    tables = build_tables_host(dem.data(), w, h, 20.0f);
    tables.attach(T);
    T.spacing_x = 30.0f;
    T.spacing_z = 25.0f;
    T.inv_spacing_x = 1.0f / T.spacing_x;
    T.inv_spacing_z = 1.0f / T.spacing_z;
    T.origin_x = -0.5f * ((float)w - 1.0f) * T.spacing_x;
    T.origin_z = -0.5f * ((float)h - 1.0f) * T.spacing_z;
    T.inv_two_r_prime = 6.7e-8f;
    T.curvature_enabled = 1u;
}
}  // namespace
