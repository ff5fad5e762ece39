"""Plain-numpy reference of the mesh BVH and a checker for every form of it.  No GPU, none of the product's code.

``lbvh_reference(vertices, indices)``: the tree ``build_mesh_lbvh`` (csrc/f3d_lbvh.hip) must emit, written from the
definition of a radix tree over sorted 64-bit keys -- top-down, a range splits at the first key that has the highest
differing bit of the range's end keys set -- not from Karras's searches.  Float32 throughout, in the builder's order of
operations (division and sqrt are correctly rounded on both sides, nothing is contracted).

``check_tree(form, nodes, tris, vertices, indices)``: what every tree a session walks must satisfy, whoever built it
(GPU LBVH, host SAH binary or collapsed four wide) and whether fresh or refitted: the leaf-order triangles are the
mesh's, the structure is a tree the walk can follow, and EVERY box is the float32 bounds of the triangles below it
-/+ the build's pad

    pad = 1e-5f * sqrt(dx*dx + dy*dy + dz*dz) + 4e-6f * max|coordinate| + 1e-30f      (bounds of the referenced vertices)

exactly.  That one rule holds at every node of every form: the host builder's top nodes and both refits take the union
of padded children, which is the padded union because x -> fl(x - pad) is monotone (f3d_bvh.h, f3d_bvh_refit.h).  Box
floats are compared by value (-0 == +0: min / max may return either zero), every other word as bits.  No tolerance.
"""
from __future__ import annotations

import numpy as np

F = np.float32
LEAF_MAX = 4
BVH4_MAX_LEVELS = 15  # f3d_scene.h kBvh4MaxLevels

NODE = np.dtype([("bmin", "<f4", 3), ("skip", "<u4"), ("bmax", "<f4", 3), ("leaf", "<u4")])
NODE4 = np.dtype([("lo_x", "<f4", 4), ("hi_x", "<f4", 4), ("lo_y", "<f4", 4), ("hi_y", "<f4", 4), ("lo_z", "<f4", 4),
                  ("hi_z", "<f4", 4), ("leaf", "<u4", 4), ("first_child", "<u4"), ("inner", "<u4"), ("pad", "<u4", 2)])
CORNER = np.dtype([("xyz", "<f4", 3), ("w", "<u4")])
assert NODE.itemsize == 32 and NODE4.itemsize == 128 and CORNER.itemsize == 16

CHECKS = ("triangles", "structure", "boxes")


# ---- shared arithmetic ---------------------------------------------------------------------------------------------------
def _mesh(vertices, indices):
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    return v, idx


def triangle_bounds(vertices, indices):
    """(lo, hi), float32 (n, 3): bounds of every triangle's three corners."""
    v, idx = _mesh(vertices, indices)
    p = v[idx]  # (n, 3 corners, xyz)
    return p.min(axis=1), p.max(axis=1)


def build_pad(lo, hi) -> np.float32:
    """The build's padding for these triangle bounds, float32 in the builder's order of operations."""
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    d = (shi - slo).astype(F)
    diag2 = F(0.0)
    for a in range(3):
        diag2 = F(diag2 + F(d[a] * d[a]))
    mag = F(max(np.abs(slo).max(), np.abs(shi).max()))
    return F(F(F(F(1e-5) * np.sqrt(diag2, dtype=F)) + F(F(4e-6) * mag)) + F(1e-30))


def _expand_bits(v):  # 10 bits -> every third bit
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for bit in range(10):
        out |= ((v >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit)
    return out


def morton_keys(vertices, indices):
    """Sorted unique keys, uint64: 30-bit Morton code of the triangle's centroid in the centroid bounds << 32 | triangle."""
    lo, hi = triangle_bounds(vertices, indices)
    c = (F(0.5) * (lo + hi)).astype(F)
    clo, chi = c.min(axis=0), c.max(axis=0)
    ext = np.maximum((chi - clo).astype(F), F(1e-6))
    with np.errstate(all="ignore"):
        u = np.clip(((c - clo).astype(F) / ext).astype(F), F(0.0), F(1.0))
    q = np.minimum(np.trunc((u * F(1023.0)).astype(F)).astype(np.uint64), np.uint64(1023))
    code = _expand_bits(q[:, 0]) | (_expand_bits(q[:, 1]) << np.uint64(1)) | (_expand_bits(q[:, 2]) << np.uint64(2))
    keys = (code << np.uint64(32)) | np.arange(len(c), dtype=np.uint64)
    return np.sort(keys)


def _msb(x):
    """Index of the highest set bit of every (non-zero) uint64."""
    x = x.copy()
    r = np.zeros(x.shape, np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(s)) != 0
        r[m] += np.uint64(s)
        x[m] >>= np.uint64(s)
    return r


def leaf_order_triangles(vertices, indices, order):
    """The leaf-order triangle records of triangles `order`: xyz of the corners, the index in corner 0's w, 0.0f elsewhere."""
    v, idx = _mesh(vertices, indices)
    order = np.asarray(order, dtype=np.int64)
    tris = np.zeros((len(order), 3), CORNER)
    tris["xyz"] = v[idx[order]]
    tris["w"][:, 0] = order.astype(np.uint32)
    return tris


# ---- the LBVH from its definition ---------------------------------------------------------------------------------------------
def lbvh_topology(keys):
    """The output tree over sorted unique keys, level by level: (skip, leaf, first, last) per node in preorder; a range
    of at most LEAF_MAX keys is a leaf, a longer one splits at the first key with the range's highest differing bit set."""
    n = len(keys)
    levels = []  # per level: first, last (inclusive), parent (position in the level above), is_right
    first, last = np.array([0], np.int64), np.array([n - 1], np.int64)
    parent, is_right = np.array([-1], np.int64), np.array([False])
    while len(first):
        inner = np.flatnonzero(last - first + 1 > LEAF_MAX)
        levels.append([first, last, parent, is_right, inner])
        if not len(inner):
            break
        a, b = first[inner], last[inner]
        p = _msb(keys[a] ^ keys[b])
        prefix = (keys[b] >> p) << p  # the smallest word with the common prefix and bit p set
        split = np.searchsorted(keys, prefix, side="left").astype(np.int64)
        assert np.all((split > a) & (split <= b))
        first = np.stack([a, split], axis=1).reshape(-1)
        last = np.stack([split - 1, b], axis=1).reshape(-1)
        parent = np.repeat(inner, 2)
        is_right = np.tile(np.array([False, True]), len(inner))
    # subtree sizes bottom-up, preorder indices top-down
    sizes = [np.ones(len(lv[0]), np.int64) for lv in levels]
    for d in range(len(levels) - 1, 0, -1):
        np.add.at(sizes[d - 1], levels[d][2], sizes[d])
    index = [np.zeros(len(lv[0]), np.int64) for lv in levels]
    for d in range(1, len(levels)):
        par = levels[d][2]
        index[d] = index[d - 1][par] + 1
        right = np.flatnonzero(levels[d][3])
        index[d][right] += sizes[d][right - 1]  # (the left sibling sits just before)
    total = int(sizes[0][0])
    skip, leaf = np.zeros(total, np.uint32), np.zeros(total, np.uint32)
    lo_key, hi_key = np.zeros(total, np.int64), np.zeros(total, np.int64)
    for d, (first, last, _, _, _) in enumerate(levels):
        i = index[d]
        skip[i] = (i + sizes[d]).astype(np.uint32)
        count = last - first + 1
        leaf[i] = np.where(count <= LEAF_MAX, (first << 3) | count, 0).astype(np.uint32)
        lo_key[i], hi_key[i] = first, last
    return skip, leaf, lo_key, hi_key


def lbvh_reference(vertices, indices):
    """(nodes, tris): the NODE records in threaded preorder and the leaf-order triangles of the linear BVH of this mesh."""
    v, idx = _mesh(vertices, indices)
    keys = morton_keys(v, idx)
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    skip, leaf, first, last = lbvh_topology(keys)
    lo, hi = triangle_bounds(v, idx)
    pad = build_pad(lo, hi)
    # bounds of every contiguous run of sorted triangles: min / max over [first, last]
    slo, shi = lo[order], hi[order]
    starts = np.stack([first, last + 1], axis=1).reshape(-1)
    ext_lo = np.concatenate([slo, np.full((1, 3), np.inf, F)])
    ext_hi = np.concatenate([shi, np.full((1, 3), -np.inf, F)])
    nodes = np.zeros(len(skip), NODE)
    nodes["skip"], nodes["leaf"] = skip, leaf
    nodes["bmin"] = (np.minimum.reduceat(ext_lo, starts, axis=0)[0::2] - pad).astype(F)
    nodes["bmax"] = (np.maximum.reduceat(ext_hi, starts, axis=0)[0::2] + pad).astype(F)
    return nodes, leaf_order_triangles(v, idx, order)


# ---- the checker -------------------------------------------------------------------------------------------------------------
class TreeReport:
    """What check_tree found: per check a list of findings ([] = passed) or None (not run: an earlier check it builds on
    failed)."""

    def __init__(self):
        self.findings = {name: None for name in CHECKS}

    def failed(self):
        return tuple(name for name in CHECKS if self.findings[name])

    @property
    def ok(self):
        return all(self.findings[name] == [] for name in CHECKS)

    def __str__(self):
        lines = []
        for name in CHECKS:
            f = self.findings[name]
            lines.append(f"{name}: " + ("not run" if f is None else "ok" if not f else "; ".join(f[:6]) + (f" (+{len(f) - 6} more)" if len(f) > 6 else "")))
        return "\n".join(lines)

    def assert_ok(self, what=""):
        assert self.ok, f"{what}\n{self}"


def _some(idx, limit=4):
    idx = np.asarray(idx).reshape(-1)
    return ", ".join(str(int(i)) for i in idx[:limit]) + (" ..." if len(idx) > limit else "")


def _check_triangles(tris, v, idx):
    out = []
    n = len(idx)
    if tris.shape != (n, 3):
        return [f"{tris.shape[0]} leaf-order triangles for a mesh of {n}"]
    w = tris["w"][:, 0]
    if np.any(w >= n):
        return [f"index word out of range at leaf-order triangles {_some(np.flatnonzero(w >= n))}"]
    seen = np.bincount(w, minlength=n)
    if np.any(seen != 1):
        out.append(f"not a permutation: triangles {_some(np.flatnonzero(seen != 1))} occur {_some(seen[seen != 1])} times")
    bad = np.flatnonzero(np.any(tris["xyz"].view(np.uint32) != v[idx[w]].view(np.uint32), axis=(1, 2)))
    if len(bad):
        out.append(f"corner positions are not the current vertices' bits at leaf-order triangles {_some(bad)}")
    bad = np.flatnonzero(np.any(tris["w"][:, 1:] != 0, axis=1))
    if len(bad):
        out.append(f"w of corner 1 or 2 is not 0.0f at leaf-order triangles {_some(bad)}")
    return out


def _check_leaf_ranges(words, n, out):
    """Leaf words (all non-zero): counts in 1..LEAF_MAX, ranges disjoint and covering [0, n)."""
    first, count = (words >> 3).astype(np.int64), (words & 7).astype(np.int64)
    bad = np.flatnonzero((count < 1) | (count > LEAF_MAX))
    if len(bad):
        out.append(f"leaf count outside 1..{LEAF_MAX}: {_some(count[bad])} (leaves {_some(bad)} of {len(words)})")
    order = np.argsort(first, kind="stable")
    f, c = first[order], count[order]
    if not len(f) or f[0] != 0 or np.any(f[1:] != (f + c)[:-1]) or f[-1] + c[-1] != n:
        out.append(f"the leaf ranges do not tile [0, {n}): {int(c.sum())} triangles in {len(f)} leaves, "
                   f"first break after range {_some(np.flatnonzero(np.append(f[1:], n) != f + c), 1)} in first-triangle order")


def _check_binary(nodes, n):
    out = []
    m = len(nodes)
    if m == 0:
        return ["no nodes"]
    skip, leaf = nodes["skip"].astype(np.int64), nodes["leaf"]
    i = np.arange(m)
    if skip[0] != m:
        out.append(f"skip[0] = {skip[0]}, node_count = {m}")
    bad = np.flatnonzero((skip <= i) | (skip > m))
    if len(bad):
        return out + [f"skip outside (i, node_count] at nodes {_some(bad)}"]
    is_leaf = leaf != 0
    bad = np.flatnonzero(is_leaf & (skip != i + 1))
    if len(bad):
        out.append(f"a leaf's skip is not the next node at nodes {_some(bad)}")
    inner = np.flatnonzero(~is_leaf)
    left = inner + 1
    bad = inner[left >= m]
    if len(bad):
        return out + [f"inner node without a first child: {_some(bad)}"]
    right = skip[left]
    ok = (right < skip[inner]) & (right < m)
    if np.any(~ok):
        out.append(f"no second child before skip at inner nodes {_some(inner[~ok])}")
    good = np.flatnonzero(ok)
    bad = inner[good][skip[right[good]] != skip[inner[good]]]
    if len(bad):
        out.append(f"the second child's skip is not its parent's at inner nodes {_some(bad)}")
    named = np.bincount(np.concatenate([left, right[good]]), minlength=m)
    bad = np.flatnonzero(named[1:] != 1) + 1
    if len(bad) or named[0] != 0:
        out.append(f"not the child of exactly one inner node: nodes {_some(bad)}" + (" (and the root is a child)" if named[0] else ""))
    if not np.any(is_leaf):
        return out + ["no leaves"]
    _check_leaf_ranges(leaf[is_leaf], n, out)
    return out


_SLOT_BOXES = ("lo_x", "lo_y", "lo_z", "hi_x", "hi_y", "hi_z")


def _wide_levels(nodes):
    """Records by level from the root: [(records, parent records, slots)]; assumes the naming was checked."""
    m = len(nodes)
    levels = [(np.array([0], np.int64), np.array([-1], np.int64), np.array([0], np.int64))]
    while True:
        recs = levels[-1][0]
        inner = nodes["inner"][recs].astype(np.int64)
        if inner.sum() == 0 or len(levels) > m:
            return levels
        par = np.repeat(recs, inner)
        slot = np.arange(inner.sum()) - np.repeat(np.cumsum(inner) - inner, inner)
        levels.append((nodes["first_child"][par].astype(np.int64) + slot, par, slot))


def _check_wide(nodes, n):
    out = []
    m = len(nodes)
    if m == 0:
        return ["no records"]
    inner, first_child, leaf = nodes["inner"].astype(np.int64), nodes["first_child"].astype(np.int64), nodes["leaf"]
    w = np.arange(m)
    bad = np.flatnonzero(inner > 4)
    if len(bad):
        return [f"more than 4 inner slots at records {_some(bad)}"]
    slots = np.arange(4)[None, :]
    is_inner = slots < inner[:, None]
    child = first_child[:, None] + slots
    bad = np.flatnonzero(np.any(is_inner & ((child <= w[:, None]) | (child >= m)), axis=1))
    if len(bad):
        return [f"an inner slot names a record outside (itself, record count) at records {_some(bad)}"]
    named = np.bincount(child[is_inner], minlength=m)
    bad = np.flatnonzero(named[1:] != 1) + 1
    if len(bad):
        out.append(f"not named exactly once: records {_some(bad)} are named {_some(named[bad])} times")
    bad = np.flatnonzero(np.any(is_inner & (leaf != 0), axis=1))
    if len(bad):
        out.append(f"an inner slot carries a leaf word at records {_some(bad)}")
    empty = ~is_inner & (leaf == 0)
    planes = np.stack([nodes[k] for k in _SLOT_BOXES], axis=-1)  # (m, 4 slots, 6)
    bad = np.flatnonzero(np.any(empty & np.any(planes != np.inf, axis=-1), axis=1))
    if len(bad):
        out.append(f"an empty slot does not hold +inf on both planes of every axis at records {_some(bad)}")
    words = leaf[~is_inner & (leaf != 0)]
    if not len(words):
        return out + ["no leaves"]
    _check_leaf_ranges(words, n, out)
    if not out:
        depth = len(_wide_levels(nodes)) - 1
        if depth > BVH4_MAX_LEVELS:
            out.append(f"records {depth} levels below the root, the walk keeps {BVH4_MAX_LEVELS}")
    return out


def _leaf_boxes(words, lo, hi):
    """Bounds of the leaf-order triangles of each leaf word: float32 (k, 3) twice."""
    first, count = (words >> 3).astype(np.int64), (words & 7).astype(np.int64)
    blo, bhi = lo[first].copy(), hi[first].copy()
    for j in range(1, LEAF_MAX):
        more = count > j
        at = np.where(more, first + j, first)
        blo, bhi = np.minimum(blo, lo[at]), np.maximum(bhi, hi[at])
    return blo, bhi


def _box_findings(what, where, got_lo, got_hi, want_lo, want_hi):
    with np.errstate(invalid="ignore"):
        bad_lo, bad_hi = np.any(got_lo != want_lo, axis=-1), np.any(got_hi != want_hi, axis=-1)
    out = []
    for name, bad, got, want in (("bmin", bad_lo, got_lo, want_lo), ("bmax", bad_hi, got_hi, want_hi)):
        at = np.flatnonzero(bad)
        if len(at):
            k = at[0]
            out.append(f"{name} of {len(at)} {what} is not bounds -/+ pad, first at {where(k)}: {got[k].tolist()} instead of {want[k].tolist()}")
    return out


def expected_binary_boxes(nodes, tris, vertices, indices, pad=None):
    """(bmin, bmax) every node of a structurally sound binary tree must hold, from the current vertices (pad: the
    build's for them unless given)."""
    v, idx = _mesh(vertices, indices)
    lo, hi = triangle_bounds(v, idx)
    pad = build_pad(lo, hi) if pad is None else F(pad)
    order = tris["w"][:, 0].astype(np.int64)
    lo, hi = lo[order], hi[order]
    m = len(nodes)
    skip, leaf = nodes["skip"].astype(np.int64), nodes["leaf"]
    want_lo, want_hi = np.full((m, 3), np.inf, F), np.full((m, 3), -np.inf, F)
    leaves = np.flatnonzero(leaf != 0)
    want_lo[leaves], want_hi[leaves] = _leaf_boxes(leaf[leaves], lo, hi)
    # depth of node i = its ancestors = the nodes j < i whose subtree has not ended: i - #{j: skip[j] <= i}
    depth = np.arange(m) - np.searchsorted(np.sort(skip), np.arange(m), side="right")
    inner = np.flatnonzero(leaf == 0)
    by_depth = inner[np.argsort(depth[inner], kind="stable")]
    cuts = np.searchsorted(depth[by_depth], np.arange(depth.max() + 2))
    for d in range(int(depth.max()), -1, -1):  # children before parents
        at = by_depth[cuts[d]:cuts[d + 1]]
        if len(at):
            a, b = at + 1, skip[at + 1]
            want_lo[at], want_hi[at] = np.minimum(want_lo[a], want_lo[b]), np.maximum(want_hi[a], want_hi[b])
    return (want_lo - pad).astype(F), (want_hi + pad).astype(F)


def _check_binary_boxes(nodes, tris, v, idx):
    want_lo, want_hi = expected_binary_boxes(nodes, tris, v, idx)
    return _box_findings("nodes", lambda k: f"node {k} (leaf word {int(nodes['leaf'][k]):#x})", nodes["bmin"], nodes["bmax"], want_lo, want_hi)


def expected_wide_boxes(nodes, tris, vertices, indices, pad=None):
    """(lo, hi), float32 (records, 4, 3): the child box every used slot of a structurally sound four-wide tree must hold
    (empty slots: +inf on both planes; pad: the build's for the current vertices unless given)."""
    v, idx = _mesh(vertices, indices)
    lo, hi = triangle_bounds(v, idx)
    pad = build_pad(lo, hi) if pad is None else F(pad)
    order = tris["w"][:, 0].astype(np.int64)
    lo, hi = lo[order], hi[order]
    m = len(nodes)
    inner, leaf = nodes["inner"].astype(np.int64), nodes["leaf"]
    is_inner = np.arange(4)[None, :] < inner[:, None]
    is_leaf = ~is_inner & (leaf != 0)
    want_lo, want_hi = np.full((m, 4, 3), np.inf, F), np.full((m, 4, 3), -np.inf, F)
    want_lo[is_leaf], want_hi[is_leaf] = _leaf_boxes(leaf[is_leaf], lo, hi)
    levels = _wide_levels(nodes)
    for recs, par, slot in reversed(levels[1:]):  # a record's union goes into its slot of the parent
        want_lo[par, slot], want_hi[par, slot] = want_lo[recs].min(axis=1), want_hi[recs].max(axis=1)
    want_lo, want_hi = (want_lo - pad).astype(F), (want_hi + pad).astype(F)
    empty = ~is_inner & ~is_leaf
    want_lo[empty] = want_hi[empty] = np.inf
    return want_lo, want_hi


def _check_wide_boxes(nodes, tris, v, idx):
    want_lo, want_hi = expected_wide_boxes(nodes, tris, v, idx)
    got_lo = np.stack([nodes[k] for k in ("lo_x", "lo_y", "lo_z")], axis=-1).reshape(-1, 3)
    got_hi = np.stack([nodes[k] for k in ("hi_x", "hi_y", "hi_z")], axis=-1).reshape(-1, 3)
    return _box_findings("child slots", lambda k: f"record {k // 4} slot {k % 4}", got_lo, got_hi, want_lo.reshape(-1, 3), want_hi.reshape(-1, 3))


def check_tree(form, nodes, tris, vertices, indices) -> TreeReport:
    """Check a tree of form 1 (NODE records, threaded preorder) or 2 (NODE4 records) with its leaf-order triangles against
    the mesh as it is now.  The checks are reported apart; `boxes` runs only on triangles and a structure that passed."""
    v, idx = _mesh(vertices, indices)
    report = TreeReport()
    if form not in (1, 2):
        report.findings["structure"] = [f"form {form}: neither 1 (binary) nor 2 (four wide)"]
        return report
    report.findings["triangles"] = _check_triangles(tris, v, idx)
    report.findings["structure"] = (_check_binary if form == 1 else _check_wide)(nodes, len(idx))
    if not report.findings["triangles"] and not report.findings["structure"]:
        report.findings["boxes"] = (_check_binary_boxes if form == 1 else _check_wide_boxes)(nodes, tris, v, idx)
    return report


def compare_trees(got_nodes, got_tris, want_nodes, want_tris):
    """Findings of a node-for-node comparison of a binary tree with the reference: counts, skip / leaf and triangle words
    as bits, box floats by value."""
    out = []
    if len(got_nodes) != len(want_nodes):
        return [f"{len(got_nodes)} nodes, the reference has {len(want_nodes)}"]
    if got_tris.shape != want_tris.shape:
        return [f"{got_tris.shape[0]} triangles, the reference has {want_tris.shape[0]}"]
    for word in ("skip", "leaf"):
        bad = np.flatnonzero(got_nodes[word] != want_nodes[word])
        if len(bad):
            out.append(f"{word} differs at {len(bad)} nodes, first {bad[0]}: {int(got_nodes[word][bad[0]])} instead of {int(want_nodes[word][bad[0]])}")
    for box in ("bmin", "bmax"):
        bad = np.flatnonzero(np.any(got_nodes[box] != want_nodes[box], axis=1))
        if len(bad):
            out.append(f"{box} differs at {len(bad)} nodes, first {bad[0]}: {got_nodes[box][bad[0]].tolist()} instead of {want_nodes[box][bad[0]].tolist()}")
    bad = np.flatnonzero(got_tris["w"][:, 0] != want_tris["w"][:, 0])
    if len(bad):
        out.append(f"the triangle order differs at {len(bad)} places, first {bad[0]}: triangle {int(got_tris['w'][bad[0], 0])} instead of {int(want_tris['w'][bad[0], 0])}")
    words = lambda t: np.ascontiguousarray(t).view(np.uint32).reshape(len(t), -1)
    bad = np.flatnonzero(np.any(words(got_tris) != words(want_tris), axis=1))
    if len(bad):
        out.append(f"triangle words differ at {len(bad)} leaf-order triangles, first {bad[0]}")
    return out


# ---- meshes the CPU and the GPU tests share ------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1000, 4097)


def soup(n, seed, scale=40.0, size=1.5, centre=(0.0, 30.0, 0.0)):
    """n unconnected triangles of about `size` scattered over +-scale around centre."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-scale, scale, (n, 1, 3)) + np.asarray(centre)
    v = (c + rng.normal(0.0, size, (n, 3, 3))).reshape(-1, 3).astype(F)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def city(n):
    """The first n triangles of a box_city large enough (its other vertices stay, unreferenced)."""
    import scenes

    v, i = scenes.box_city(n_boxes=max(1, -(-n // 12)), seed=5)
    assert len(i) >= n
    return v, i[:n].copy()


def edge_meshes():
    """{name: (vertices, indices)}: the inputs at which a Morton-code builder takes its special paths."""
    out = {}
    one = np.asarray([[1.0, 20.0, 2.0], [4.0, 22.0, 2.5], [2.0, 25.0, 6.0]], F)
    for reps in (37, 300):  # all codes equal: the tree comes from the index bits alone
        out[f"one_triangle_x{reps}"] = (one.copy(), np.tile(np.arange(3, dtype=np.uint32), (reps, 1)))
    gx, gz = 9, 7  # a flat grid in one plane: the y extent of the centroids is 0, floored at 1e-6
    x, z = np.meshgrid(np.linspace(-20.0, 20.0, gx + 1), np.linspace(-15.0, 15.0, gz + 1))
    v = np.stack([x, np.full_like(x, 12.5), z], axis=-1).reshape(-1, 3).astype(F)
    a = (np.arange(gz)[:, None] * (gx + 1) + np.arange(gx)[None, :]).reshape(-1)
    out["flat_grid"] = (v, np.concatenate([np.stack([a, a + 1, a + gx + 1], 1), np.stack([a + 1, a + gx + 2, a + gx + 1], 1)]).astype(np.uint32))
    va, ia = soup(150, 11, scale=0.02, size=0.004, centre=(0.0, 20.0, 0.0))  # two tight clusters 1e4 apart: runs of equal codes, a large pad
    vb, ib = soup(150, 12, scale=0.02, size=0.004, centre=(1e4, 20.0, 1e4))
    out["two_clusters"] = (np.concatenate([va, vb]), np.concatenate([ia, ib + len(va)]).astype(np.uint32))
    v, i = soup(100, 13)  # several centroids exactly on the centroid bounds: u == 0 and u == 1, q clamped to 1023
    lo, hi = triangle_bounds(v, i)
    c = F(0.5) * (lo + hi)
    corners = []
    for p in (c.min(axis=0) - F(2.0), c.max(axis=0) + F(2.0)):
        for _ in range(3):
            corners += [p - F(0.5), p, p + F(0.5)]  # (bounds p -/+ 0.5: the centroid is p exactly)
    v2 = np.concatenate([v, np.asarray(corners, F)])
    out["centroids_on_the_bounds"] = (v2, np.concatenate([i, np.arange(len(v), len(v2), dtype=np.uint32).reshape(-1, 3)]))
    rng = np.random.default_rng(14)  # zero-area and sliver triangles
    p = rng.uniform(-30.0, 30.0, (60, 3)).astype(F) + F([0.0, 40.0, 0.0])
    d = rng.normal(0.0, 5.0, (60, 3)).astype(F)
    tri = np.stack([p, p + d, p + d * F(2.0)], axis=1)       # collinear
    tri[:20, 1] = tri[:20, 2] = tri[:20, 0]                   # a point
    tri[20:40, 2] = tri[20:40, 1] + F(1e-4)                   # a sliver
    out["degenerate"] = (tri.reshape(-1, 3).astype(F), np.arange(180, dtype=np.uint32).reshape(60, 3))
    return out


def displaced_grid(cells=318, seed=3):
    """A displaced grid of 2 * cells^2 triangles (202 248 by default) hanging over the golden scene's footprint."""
    rng = np.random.default_rng(seed)
    x, z = np.meshgrid(np.linspace(-45.0, 45.0, cells + 1), np.linspace(-45.0, 45.0, cells + 1))
    y = 32.0 + 3.0 * np.sin(0.3 * x) * np.cos(0.2 * z) + rng.uniform(-0.3, 0.3, x.shape)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)
    a = (np.arange(cells)[:, None] * (cells + 1) + np.arange(cells)[None, :]).reshape(-1)
    i = np.concatenate([np.stack([a, a + 1, a + cells + 1], 1), np.stack([a + 1, a + cells + 2, a + cells + 1], 1)]).astype(np.uint32)
    return v, i
