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
}  // namespace
