"""CPU: the numpy BVH reference and checker of bvh_reference.py can fail.

The reference tree of ~20 seeded meshes passes the checker in both forms; its topology is cross-checked from the keys'
common prefixes alone; and each single mutation of a good tree -- the faults a builder or a refit kernel could leave
behind -- is reported by the check it belongs to and by no other.
"""
from __future__ import annotations

import numpy as np
import pytest

import bvh_reference as R
import scenes

F = np.float32


def collapse4(nodes):
    """The binary tree four children wide, as Bvh4Node documents it: a record adopts the children of its largest inner
    child until it has four; inner children first, as the consecutive records first_child + slot; the children's boxes
    live in the parent; unused slots hold +inf on both planes and a leaf word of 0."""
    skip, leaf = nodes["skip"].astype(np.int64), nodes["leaf"]

    def area(b):
        dx, dy, dz = (nodes["bmax"][b] - nodes["bmin"][b]).tolist()
        return dx * dy + dy * dz + dz * dx

    out = []

    def record():
        rec = np.zeros((), R.NODE4)
        for k in ("lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z"):
            rec[k] = np.inf
        out.append(rec)
        return len(out) - 1

    def fill(rec, slot, b):
        for a, axis in enumerate("xyz"):
            rec["lo_" + axis][slot], rec["hi_" + axis][slot] = nodes["bmin"][b][a], nodes["bmax"][b][a]
        rec["leaf"][slot] = leaf[b]

    record()
    if leaf[0] != 0:
        fill(out[0], 0, 0)
        return np.asarray(out, R.NODE4)
    todo = [(0, 0)]
    while todo:
        b, w = todo.pop()
        kids = [b + 1, int(skip[b + 1])]
        while len(kids) < 4:
            inner = [k for k in kids if leaf[k] == 0]
            if not inner:
                break
            pick = max(inner, key=area)
            kids[kids.index(pick)] = pick + 1
            kids.append(int(skip[pick + 1]))
        order = [k for k in kids if leaf[k] == 0] + [k for k in kids if leaf[k] != 0]
        n_inner = sum(1 for k in kids if leaf[k] == 0)
        first_child = len(out)
        for _ in range(n_inner):
            record()
        for slot, k in enumerate(order):
            fill(out[w], slot, k)
        out[w]["first_child"], out[w]["inner"] = first_child, n_inner
        todo += [(k, first_child + slot) for slot, k in enumerate(order[:n_inner])]
    return np.asarray(out, R.NODE4)


def _meshes():
    out = {}
    for seed in (1, 2, 3, 4):
        out[f"box_city_{seed}"] = scenes.box_city(n_boxes=4 + 9 * seed, seed=seed)
        out[f"blob_{seed}"] = scenes._blob_mesh(np.random.default_rng(seed), n_lat=3 + seed, n_lon=5 + seed)
    for n in (1, 4, 5, 65, 257, 1000):
        out[f"soup_{n}"] = R.soup(n, 100 + n)
    out["city_63"] = R.city(63)
    out.update(R.edge_meshes())
    return out


MESHES = _meshes()
_TREES = {}


def _tree(name):
    if name not in _TREES:
        v, i = MESHES[name]
        nodes, tris = R.lbvh_reference(v, i)
        for a in (nodes, tris):
            a.setflags(write=False)
        _TREES[name] = (nodes, tris)
    return _TREES[name]


def test_the_set_of_meshes_is_about_twenty():
    assert 18 <= len(MESHES) <= 24


@pytest.mark.parametrize("name", sorted(MESHES))
def test_reference_trees_pass_the_checker_in_both_forms(name):
    v, i = MESHES[name]
    nodes, tris = _tree(name)
    assert nodes["skip"][0] == len(nodes) and tris.shape == (len(i), 3)
    R.check_tree(1, nodes, tris, v, i).assert_ok(f"{name}, binary")
    R.check_tree(2, collapse4(nodes), tris, v, i).assert_ok(f"{name}, four wide")
    assert R.compare_trees(nodes, tris, nodes.copy(), tris.copy()) == []


def _prefix(a, b):
    return 64 - int(int(a) ^ int(b)).bit_length()


@pytest.mark.parametrize("name", sorted(MESHES))
def test_reference_topology_from_common_prefixes(name):
    """Independent of the top-down construction: every node of a radix tree covers a maximal run of keys -- the keys of
    the run share a longer prefix with each other than with the key before or after it -- and its children cut the run
    where that shared prefix ends; every run of more than 4 keys is split, no run of at most 4 is."""
    v, i = MESHES[name]
    nodes, tris = _tree(name)
    keys = R.morton_keys(v, i)
    assert len(np.unique(keys)) == len(keys) == len(i)
    assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), tris["w"][:, 0])
    skip, leaf = nodes["skip"].astype(np.int64), nodes["leaf"]
    # the run of every node: from the first triangle of its first leaf to the last of its last one
    is_leaf = leaf != 0
    at = np.flatnonzero(is_leaf)
    first_of, end_of = (leaf[at] >> 3).astype(np.int64), (leaf[at] >> 3).astype(np.int64) + (leaf[at] & 7)
    assert np.array_equal(first_of[1:], end_of[:-1])  # (the builder's leaves are in key order along the preorder)
    first = first_of[np.searchsorted(at, np.arange(len(nodes)), side="left")]
    last = end_of[np.searchsorted(at, skip - 1, side="right") - 1] - 1
    n = len(keys)
    for k in range(len(nodes)):
        a, b = int(first[k]), int(last[k])
        assert (b - a + 1 <= R.LEAF_MAX) == bool(is_leaf[k]), k
        inside = _prefix(keys[a], keys[b]) if b > a else 64
        if a > 0:
            assert _prefix(keys[a - 1], keys[a]) < inside, k
        if b < n - 1:
            assert _prefix(keys[b], keys[b + 1]) < inside, k
        if not is_leaf[k]:
            l, r = k + 1, int(skip[k + 1])
            assert first[l] == a and last[l] + 1 == first[r] and last[r] == b, k
            assert _prefix(keys[last[l]], keys[first[r]]) == inside, k  # the cut is where the shared prefix ends


# ---- mutations ---------------------------------------------------------------------------------------------------------------
def _moved(v, how):
    rng = np.random.default_rng(5)
    if how == "jitter":
        return (v + rng.uniform(-2.0, 2.0, v.shape)).astype(F)
    return (v + F(1e4)).astype(F)  # "away": the pad is another


def _good(form, moved=None):
    """A sound tree of box_city(30, 5) in this form (writable copies), fresh or refitted to moved vertices; with the mesh."""
    v, i = scenes.box_city(n_boxes=30, seed=5)
    nodes, tris = R.lbvh_reference(v, i)
    if form == 2:
        nodes = collapse4(nodes)
    if moved is not None:
        nodes, tris = _refit(form, nodes, tris, _moved(v, moved), i)
        v = _moved(v, moved)
    return nodes, tris, v, i


def _refit(form, nodes, tris, v, i, pad=None):
    """What a refit leaves: the topology words kept, the triangles read again, every box from the new positions."""
    nodes = nodes.copy()
    tris = R.leaf_order_triangles(v, i, tris["w"][:, 0])
    if form == 1:
        nodes["bmin"], nodes["bmax"] = R.expected_binary_boxes(nodes, tris, v, i, pad)
    else:
        lo, hi = R.expected_wide_boxes(nodes, tris, v, i, pad)
        for a, axis in enumerate("xyz"):
            nodes["lo_" + axis], nodes["hi_" + axis] = lo[:, :, a], hi[:, :, a]
    return nodes, tris


def _boxes(form, nodes):
    """(views of) the min planes and the max planes of a tree, and an index of a used box in them."""
    if form == 1:
        return nodes["bmin"], nodes["bmax"], (len(nodes) // 2, 1)
    rec = int(np.flatnonzero(nodes["inner"] > 0)[-1])
    return nodes["lo_y"], nodes["hi_y"], (rec, 0)


FORMS = pytest.mark.parametrize("form", (1, 2))


@FORMS
@pytest.mark.parametrize("moved", (None, "jitter", "away"))
def test_sound_trees_fresh_and_refitted_pass(form, moved):
    nodes, tris, v, i = _good(form, moved)
    R.check_tree(form, nodes, tris, v, i).assert_ok()


@FORMS
def test_one_bmin_raised_by_one_ulp_is_a_box_finding(form):
    nodes, tris, v, i = _good(form)
    lo, _, at = _boxes(form, nodes)
    lo[at] = np.nextafter(lo[at], F(np.inf))  # too narrow: the walk may cull a triangle the sweep would hit
    assert R.check_tree(form, nodes, tris, v, i).failed() == ("boxes",)


@FORMS
def test_one_bmax_raised_by_one_ulp_is_a_box_finding(form):
    nodes, tris, v, i = _good(form)
    _, hi, at = _boxes(form, nodes)
    hi[at] = np.nextafter(hi[at], F(np.inf))  # too wide: no image ever shows it
    assert R.check_tree(form, nodes, tris, v, i).failed() == ("boxes",)


@FORMS
def test_a_parent_box_left_from_before_a_motion_is_a_box_finding(form):
    old, _, _, _ = _good(form)
    nodes, tris, v, i = _good(form, "jitter")
    if form == 1:
        k = int(np.flatnonzero(nodes["leaf"] == 0)[3])  # an inner node
        assert np.any(nodes["bmin"][k] != old["bmin"][k])
        nodes["bmin"][k], nodes["bmax"][k] = old["bmin"][k], old["bmax"][k]
    else:
        k = int(np.flatnonzero(nodes["inner"] > 0)[1])  # an inner child's box in its parent
        assert np.any(nodes["lo_x"][k, 0] != old["lo_x"][k, 0])
        for key in ("lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z"):
            nodes[key][k, 0] = old[key][k, 0]
    assert R.check_tree(form, nodes, tris, v, i).failed() == ("boxes",)


@FORMS
def test_the_pad_of_the_old_bounds_is_a_box_finding(form):
    nodes, tris, v, i = _good(form)
    lo, hi = R.triangle_bounds(v, i)
    old_pad = R.build_pad(lo, hi)
    far = _moved(v, "away")
    assert R.build_pad(*R.triangle_bounds(far, i)) > old_pad
    nodes, tris = _refit(form, nodes, tris, far, i, pad=old_pad)
    assert R.check_tree(form, nodes, tris, far, i).failed() == ("boxes",)


def test_one_skip_off_by_one_is_a_structure_finding():
    nodes, tris, v, i = _good(1)
    k = int(np.flatnonzero(nodes["leaf"] == 0)[5])
    for step in (1, -1):
        bad = nodes.copy()
        bad["skip"][k] = int(bad["skip"][k]) + step
        assert R.check_tree(1, bad, tris, v, i).failed() == ("structure",)
    bad = nodes.copy()
    bad["skip"][np.flatnonzero(nodes["leaf"] != 0)[2]] += 1  # a leaf that jumps the node after it
    assert R.check_tree(1, bad, tris, v, i).failed() == ("structure",)


def test_two_leaves_with_their_ranges_swapped_is_a_box_finding():
    """Still a tiling of [0, n) -- the structure is sound -- but each of the two boxes now bounds the other's triangles."""
    nodes, tris, v, i = _good(1)
    a, b = np.flatnonzero(nodes["leaf"] != 0)[[1, 7]]
    assert np.any(nodes["bmin"][a] != nodes["bmin"][b])
    nodes["leaf"][[a, b]] = nodes["leaf"][[b, a]]
    assert R.check_tree(1, nodes, tris, v, i).failed() == ("boxes",)


@FORMS
def test_one_triangle_duplicated_over_another_is_a_triangle_finding(form):
    nodes, tris, v, i = _good(form)
    tris[10] = tris[200]
    assert R.check_tree(form, nodes, tris, v, i).failed() == ("triangles",)


def test_triangle_words_are_compared_as_bits():
    nodes, tris, v, i = _good(1)
    for mutate in (lambda t: t["w"].__setitem__((5, 1), 1),                                   # w of corner 1 not 0.0f
                   lambda t: t["xyz"].__setitem__((5, 2, 0), np.nextafter(t["xyz"][5, 2, 0], F(np.inf))),  # a stale position
                   lambda t: t["w"].__setitem__((5, 0), len(i))):                             # an index past the mesh
        bad = tris.copy()
        mutate(bad)
        assert R.check_tree(1, nodes, bad, v, i).failed() == ("triangles",)
    assert R.check_tree(1, nodes, tris[:-1], v, i).failed() == ("triangles",)


@FORMS
def test_a_leaf_count_of_five_is_a_structure_finding(form):
    nodes, tris, v, i = _good(form)
    words = nodes["leaf"]
    at = tuple(np.argwhere((words != 0) & ((words & 7) == 4))[0])
    words[at] += 1
    assert R.check_tree(form, nodes, tris, v, i).failed() == ("structure",)


def test_a_wide_record_named_twice_is_a_structure_finding():
    nodes, tris, v, i = _good(2)
    recs = np.flatnonzero(nodes["inner"] > 0)
    a, b = int(recs[1]), int(recs[2])
    nodes["first_child"][a] = nodes["first_child"][b]  # a's children are never named, b's twice
    assert R.check_tree(2, nodes, tris, v, i).failed() == ("structure",)


def test_wide_conventions_are_structure_findings():
    nodes, tris, v, i = _good(2)
    rec, slot = np.argwhere((np.arange(4)[None, :] >= nodes["inner"][:, None]) & (nodes["leaf"] == 0))[0]
    bad = nodes.copy()
    bad["hi_z"][rec, slot] = -np.inf  # the "inverted" empty box passes the walk's slab test for every ray
    assert R.check_tree(2, bad, tris, v, i).failed() == ("structure",)
    bad = nodes.copy()
    rec = int(np.flatnonzero(nodes["inner"] > 0)[0])
    bad["leaf"][rec, 0] = (3 << 3) | 1  # an inner slot with a leaf word
    assert R.check_tree(2, bad, tris, v, i).failed() == ("structure",)


def _chain4(n):
    """A four-wide tree over n triangles that is one chain: every record one inner child and a leaf of one triangle, the
    last record two leaves; its deepest record is n - 2 levels below the root."""
    vs, idx = R.soup(n, 9)
    chain = np.zeros(n - 1, R.NODE4)
    for key in ("lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z"):
        chain[key] = np.inf
    for w in range(n - 1):
        last = w == n - 2
        chain["inner"][w], chain["first_child"][w] = (0, 0) if last else (1, w + 1)
        chain["leaf"][w, 0 if last else 1] = (w << 3) | 1
        if last:
            chain["leaf"][w, 1] = ((w + 1) << 3) | 1
    chain, tris = _refit(2, chain, R.leaf_order_triangles(vs, idx, np.arange(n)), vs, idx)
    return chain, tris, vs, idx


def test_a_wide_tree_deeper_than_the_walks_stack_is_a_structure_finding():
    R.check_tree(2, *_chain4(R.BVH4_MAX_LEVELS + 2)).assert_ok()
    report = R.check_tree(2, *_chain4(R.BVH4_MAX_LEVELS + 3))
    assert report.failed() == ("structure",) and "levels" in str(report)


def test_compare_trees_reports_each_kind_of_word():
    nodes, tris, v, i = _good(1)
    for field, at, value in (("skip", 3, 0), ("leaf", 2, 0xFFFF), ("bmin", (4, 1), -1e9), ("bmax", (4, 2), 1e9)):
        bad = nodes.copy()
        bad[field][at] = value
        found = R.compare_trees(bad, tris, nodes, tris)
        assert len(found) == 1 and found[0].startswith(field), found
    bad = tris.copy()
    bad[[3, 4]] = bad[[4, 3]]
    assert len(R.compare_trees(nodes, bad, nodes, tris)) == 2  # the order and the words
    assert R.compare_trees(nodes[:-1], tris, nodes, tris) and R.compare_trees(nodes, tris[:-1], nodes, tris)
    zero = nodes.copy()
    zero["bmin"][0, 0] = F(0.0)
    minus = zero.copy()
    minus["bmin"][0, 0] = F(-0.0)
    assert R.compare_trees(minus, tris, zero, tris) == []  # box floats by value
