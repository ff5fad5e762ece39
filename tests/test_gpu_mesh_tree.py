"""`-m gpu`: the mesh BVH a session walks, read back (f3d_session_mesh_tree) and checked at every node.

Images cannot see most of what can go wrong in a culling structure -- a box left too wide never shows, a box too narrow
or a `skip` past a subtree only where a sample ray crosses exactly that triangle -- so these tests look at the tree
itself, against tests/bvh_reference.py (plain numpy, none of the product's code):

  * the GPU linear-BVH builder (csrc/f3d_lbvh.hip: k_prims, k_keys, the rocPRIM sort, k_link, k_refit, k_emit) equals the
    reference node for node -- node count, every skip / leaf word, every box, the triangle order and words -- at the
    sizes around the kernels' block edges and on the inputs where a Morton-code builder takes its special paths;
  * every builder's fresh tree (host SAH uploaded four wide or binary, GPU LBVH) passes check_tree: the triangles are
    the mesh's, the structure is sound, every box is the float32 bounds of the triangles below it -/+ the build's pad;
  * under real concurrency (a displaced grid of 202 248 triangles: the bottom-up passes run ~600 workgroups of 256)
    the same, and through a chain of GPU refits (csrc/f3d_bvh_refit.hip) -- jitter, 1e4 away, back -- the topology words
    never change and every box is the rule's for the positions of the moment, the pad (computed on the device) included;
  * the picture of the refitted session is still the fresh session's, and the entry's refusals.

No tolerance anywhere: box floats are compared by value, every other word as bits.

Not covered: triangles with an index past the vertex count cannot reach the builder (f3d_setup.h refuses the mesh), so
its `valid` compaction -- the sentinel keys that sort behind every real one -- stays untested here.  Nothing here reads
the oracle.

Cost of the Python side for the large mesh, measured on the development CPU: lbvh_reference 0.44 s, one check_tree
0.22 s (151 419 nodes).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import bvh_reference as R
import scenes

pytestmark = pytest.mark.gpu

W = H = 16
EDGES = R.edge_meshes()
F = np.float32


def _scene():
    dem = scenes.golden_dem(8)
    return dem, dict(scenes.CAM), scenes.fixed_frames(scenes.scene_kwargs(dem), 2)


def _session(mesh=None, builder=0):
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = _scene()
    if mesh is not None:
        kw = dict(kw, mesh_vertices=mesh[0], mesh_indices=mesh[1])
    return TerrainSession(dem, W, H, cam, mesh_builder=builder, **kw)


def _read(s, builder):
    """The session's tree, in the form its builder promises, in the reference's record types."""
    form, nodes, tris = s.mesh_tree()
    assert form == (2 if builder == 1 else 1), f"builder {builder} walks form {form}"
    assert nodes.dtype.itemsize == (128 if form == 2 else 32) and tris.dtype.itemsize == 16
    return form, nodes.view(R.NODE4 if form == 2 else R.NODE), tris.view(R.CORNER)


def _equals_reference(mesh, what):
    want_nodes, want_tris = R.lbvh_reference(*mesh)
    with _session(mesh, 2) as s:
        form, nodes, tris = _read(s, 2)
    print(f"{what}: {len(mesh[1])} triangles, {len(nodes)} nodes (reference {len(want_nodes)})")
    assert R.compare_trees(nodes, tris, want_nodes, want_tris) == [], what
    R.check_tree(form, nodes, tris, *mesh).assert_ok(what)


@pytest.mark.parametrize("n", R.SIZES)
def test_lbvh_equals_the_reference_on_a_triangle_soup(n):
    _equals_reference(R.soup(n, 1000 + n), f"soup of {n}")


@pytest.mark.parametrize("n", R.SIZES)
def test_lbvh_equals_the_reference_on_a_box_city(n):
    _equals_reference(R.city(n), f"box city cut to {n}")


@pytest.mark.parametrize("name", sorted(EDGES))
def test_lbvh_equals_the_reference_on_edge_meshes(name):
    _equals_reference(EDGES[name], name)


@pytest.mark.parametrize("builder", (1, 2, 3))
def test_every_builders_fresh_tree_passes_the_checker(builder):
    mesh = scenes.box_city(n_boxes=30, seed=5)
    with _session(mesh, builder) as s:
        form, nodes, tris = _read(s, builder)
    print(f"builder {builder}: form {form}, {len(nodes)} records")
    R.check_tree(form, nodes, tris, *mesh).assert_ok(f"builder {builder}")


@pytest.mark.parametrize("builder", (1, 2, 3))
def test_a_refit_writes_the_sessions_own_tree_and_never_the_shared_one(builder):
    """The read-back follows params.mesh: the refitted session's own copy; another session on the cached mesh sees the
    tree as it was built."""
    v, i = scenes.box_city(n_boxes=30, seed=5)
    moved = (v + np.random.default_rng(7).uniform(-3.0, 3.0, v.shape)).astype(F)
    with _session((v, i), builder) as s, _session((v, i), builder) as other:
        form, fresh_nodes, fresh_tris = _read(s, builder)
        s.remesh(moved)
        _, nodes, tris = _read(s, builder)
        R.check_tree(form, nodes, tris, moved, i).assert_ok(f"builder {builder}, refitted")
        _, other_nodes, other_tris = _read(other, builder)
        assert other_nodes.tobytes() == fresh_nodes.tobytes() and other_tris.tobytes() == fresh_tris.tobytes()
        R.check_tree(form, other_nodes, other_tris, v, i).assert_ok(f"builder {builder}, the shared tree")


# ---- under concurrency: ~200 000 triangles, fresh and through a chain of refits -----------------------------------------------
_LARGE = {}


def _large():
    if not _LARGE:
        v, i = R.displaced_grid()
        assert len(i) >= 131072
        rng = np.random.default_rng(2024)
        _LARGE.update(mesh=(v, i), reference=R.lbvh_reference(v, i),
                      jitter=(v + rng.uniform(-0.2, 0.2, v.shape)).astype(F), away=(v + F(1e4)).astype(F))
        for a in (v, i, *_LARGE["reference"], _LARGE["jitter"], _LARGE["away"]):
            a.setflags(write=False)
    return _LARGE


def _topology(form, nodes, tris):
    words = ("leaf", "first_child", "inner") if form == 2 else ("skip", "leaf")
    return tuple(nodes[w].tobytes() for w in words) + (tris["w"].tobytes(),)


def _box_planes(form, nodes):
    return [nodes[k] for k in (("lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z") if form == 2 else ("bmin", "bmax"))]


@pytest.mark.parametrize("builder", (2, 1, 3))
def test_large_mesh_fresh_and_through_a_chain_of_refits(builder):
    from test_gpu_remesh import _same

    large = _large()
    v, i = large["mesh"]
    ref_nodes, ref_tris = large["reference"]
    with _session((v, i), builder) as s:
        form, nodes, tris = _read(s, builder)
        print(f"builder {builder}: {len(i)} triangles, form {form}, {len(nodes)} records")
        if builder == 2:
            assert R.compare_trees(nodes, tris, ref_nodes, ref_tris) == [], "fresh"
        R.check_tree(form, nodes, tris, v, i).assert_ok("fresh")
        fresh_nodes, topology = nodes, _topology(form, nodes, tris)
        # jitter: the first refit (links derived, counters from zero); away: the other set of bounds, the counters the
        # first refit left, a pad dominated by the magnitude term; back: the first set of bounds again
        for motion, moved in (("jitter", large["jitter"]), ("away", large["away"]), ("back", v)):
            s.remesh(moved)
            _, nodes, tris = _read(s, builder)
            assert _topology(form, nodes, tris) == topology, f"{motion}: a refit changed a topology word"
            R.check_tree(form, nodes, tris, moved, i).assert_ok(motion)
        if builder == 2:
            assert R.compare_trees(nodes, tris, ref_nodes, ref_tris) == [], "back"
        for got, want in zip(_box_planes(form, nodes), _box_planes(form, fresh_nodes)):
            assert np.array_equal(got, want), "back: a box is not the fresh tree's"
        # the picture still agrees: what was read back is what is rendered
        got = s.render()
    with _session((v, i), builder) as fresh:
        _same(got, fresh.render(), f"builder {builder}: refitted there and back vs a fresh session")


# ---- the entry's own contract ---------------------------------------------------------------------------------------------------
def test_a_session_without_a_mesh_has_no_tree():
    with _session() as s:
        form, nodes, tris = s.mesh_tree()
    assert form == 0 and len(nodes) == 0 and tris.shape == (0, 3)


def test_sizes_capacities_and_handles():
    from forge3d_amd import _native

    L = _native.lib()
    v, i = scenes.box_city(n_boxes=30, seed=5)
    err = C.create_string_buffer(512)
    info = (C.c_uint32 * 4)()
    for builder in (1, 2, 3):
        s = _session((v, i), builder)
        form, nodes, tris = s.mesh_tree()
        assert L.f3d_session_mesh_tree(s._handle, info, None, 0, None, 0, err, len(err)) == 0  # null buffers: the sizes only
        assert list(info) == [form, len(nodes), len(i), 0]  # (the triangle count of the leaf-order buffer's bytes)
        for short_nodes, short_tris, named in ((1, 0, b"node buffer"), (0, 1, b"triangle buffer")):
            n2, t2 = np.zeros_like(nodes), np.zeros_like(tris)
            rc = L.f3d_session_mesh_tree(s._handle, info, n2.ctypes.data, n2.nbytes - short_nodes, t2.ctypes.data, t2.nbytes - short_tris,
                                         err, len(err))
            assert rc == _native.STATUS_VALUE and named in err.value, (rc, err.value)
            assert not n2.tobytes().strip(b"\0") and not t2.tobytes().strip(b"\0")  # refused before anything is written
        n2 = np.zeros_like(nodes)
        assert L.f3d_session_mesh_tree(s._handle, info, n2.ctypes.data, n2.nbytes, None, 0, err, len(err)) == 0  # one buffer alone
        assert n2.tobytes() == nodes.tobytes()
        s.close()
        with pytest.raises(ValueError, match="null session handle"):
            s.mesh_tree()
    assert L.f3d_session_mesh_tree(None, info, None, 0, None, 0, err, len(err)) == _native.STATUS_VALUE
    assert b"null session handle" in err.value
