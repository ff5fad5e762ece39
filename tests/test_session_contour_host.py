"""Contour lines on a live terrain session (f3d_session_contours, f3d_session_paint_contours), the parts that need no GPU.

The lane bodies of the contour kernels (csrc/f3d_contour.h, what k_contour_count and k_contour_emit run per lane) compiled for
the host (tests/contour_host) and run over whole 64-lane waves -- count, scan, emit -- against tests/contour_reference.py, an
independent float64 statement of the contract that loops over cells and knows nothing of blocks, bands or waves.

* DEMs 2x2, 5x3, 9x9, 10x9, 33x33 at (10, 7) m, 64x64 and 65x63 (contour_cases.SHAPES), exaggeration 1 and 2.5; regions whole, one
  cell, strictly inside a block, across block borders unaligned; level lists of one level, an interval, the maximum count
  (a steep cell crosses thousands), all below, all above, at the minimum, at the maximum, at a sample's height;
* the sequence of (cell, level, case) is the reference's EXACTLY -- `h >= level` on float32 values is the same comparison in
  float64 --, in block order, with and without the band cull;
* coordinates: |p - p64| / max(|p64|, spacing) <= TOL = 8 x the largest ratio MEASURED over exactly these inputs (below, and
  DESIGN.md) -- a few 2^-24 by derivation: three roundings in t, each scaled by at most the spacing, two in the position,
  plane_at's own;
* known answers: a planar ramp, a checkerboard (every cell a saddle), a plateau at the level, the cone h = 400 - r at a level
  between samples (one closed loop within 1 % of 2 pi r) and through samples (crossings coincide in fours and sixes);
* shared ends: where no level equals a sample every crossing off the region's border is the end of exactly two segments, bit
  for bit; chain_contours on hand-made inputs;
* a stand-alone driver (its own main) of the same lane bodies built with -fsanitize=address,undefined and run once;
* the header, the ctypes table, the descriptors' layout and INTEGRATION.md's structs; the wrapper's methods and checks.
The refusals of the two entry points need a session, i.e. a device: tests/test_gpu_contour.py.
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import contour_cases as cases
import contour_reference as ref
from emul import emul
from test_session_raster_host import plane_at
from test_session_rearm_host import _no_device

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
ULP = 2.0 ** -24

# The largest |p - p64| / max(|p64|, spacing) of the host body against the float64 reference over SHAPES x EXAGGERATIONS x
# regions x level lists, measured (test_host_body_against_the_reference prints each shape's).  The bound is 8 x it -- the
# project's margin: the measured maximum is one draw of a rounding error whose worst case over other inputs is a small multiple
# of it.  By derivation it is a few units of 2^-24; above about ten units it would contradict the derivation.
MEASURED = 1.24e-7  # = 2.07 x 2^-24: 64x64, exaggeration 2.5
TOL = 8.0 * MEASURED


@pytest.fixture(scope="module")
def harness():
    return cases.build_harness()


def _scene(harness, shape, spacing, exaggeration, dem=None):
    dem = cases.shaped_dem(shape) if dem is None else dem
    return cases.HostContours(harness, dem, cases.shape_kw(dem, spacing, exaggeration))


def _ratio(scene, got, want64):
    """The largest |p - p64| / max(|p64|, spacing) over the coordinates of got (N, 4) f32 against want64 (N, 4) f64."""
    if len(got) == 0:
        return 0.0
    sp = np.array([scene.spacing[0], scene.spacing[1]] * 2, np.float64)
    return float((np.abs(got.astype(np.float64) - want64) / np.maximum(np.abs(want64), sp)).max())


def _check_against_reference(scene, levels, region, cull=True):
    got = scene.run(levels, region, cull=cull, details=True)
    want = ref.block_order(ref.contours(scene.heights, scene.origin, scene.spacing, levels, region), scene.cell_w)
    assert got["total"] == len(want["cell"]) == len(got["segments"])
    assert np.array_equal(got["cell"], want["cell"]) and np.array_equal(got["level_index"], want["level_index"])
    assert np.array_equal(got["case"], want["case"])
    assert np.isfinite(got["segments"]).all()
    return got, _ratio(scene, got["segments"], want["xz"])


@pytest.mark.parametrize("exaggeration", cases.EXAGGERATIONS)
@pytest.mark.parametrize("shape,spacing", cases.SHAPES, ids=[f"{s[1]}x{s[0]}" for s, _ in cases.SHAPES])
def test_host_body_against_the_reference(harness, shape, spacing, exaggeration):
    scene = _scene(harness, shape, spacing, exaggeration)
    try:
        assert np.array_equal(scene.heights, ref.session_heights(scene.dem, exaggeration)), "the leaf table holds f32(h * exaggeration)"
        small = shape[0] * shape[1] <= 81
        lists = cases.level_lists(scene.heights, steep=small)
        worst, segments = 0.0, 0
        for rname, region in cases.regions(shape).items():
            for lname, levels in lists.items():
                if lname == "maximum count" and rname != "whole":
                    continue
                got, ratio = _check_against_reference(scene, levels, region)
                worst, segments = max(worst, ratio), segments + got["total"]
                if lname in ("below", "above"):
                    assert got["total"] == 0
                if lname == "maximum count":
                    assert len(levels) == 65536 and np.bincount(got["cell"]).max() > 64, "a cell crosses more than 64 levels"
                if lname == "at the minimum":
                    assert got["total"] == 0, "h >= min everywhere: every cell is case 15"
        print(f"{shape[1]}x{shape[0]} x{exaggeration}: {segments} segments, worst ratio {worst:.3e} = {worst / ULP:.2f} x 2^-24")
        assert worst <= TOL
        assert MEASURED <= 10.0 * ULP, "the derivation: a few units of 2^-24"
    finally:
        scene.close()


@pytest.mark.parametrize("shape,spacing", [cases.SHAPES[1], cases.SHAPES[3], cases.SHAPES[6]], ids=["5x3", "10x9", "65x63"])
def test_the_order_depends_on_nothing_but_the_cells(harness, shape, spacing):
    """The cull, the region's alignment and a capacity change nothing: a region's records are the whole DEM's records of its
    cells, in their order; no cull returns the same bits; a capacity returns the prefix."""
    scene = _scene(harness, shape, spacing, 2.5)
    try:
        levels = cases.level_lists(scene.heights, steep=False)["interval"]
        whole = scene.run(levels, details=True)
        assert whole["total"] > 0
        for region in cases.regions(shape).values():
            row0, col0, rows, cols = region
            part = scene.run(levels, region, details=True)
            plain = scene.run(levels, region, cull=False, details=True)
            for key in ("segments", "level_index", "cell"):
                assert part[key].tobytes() == plain[key].tobytes(), "the band cull drops nothing and moves nothing"
            cz, cx = whole["cell"] // scene.cell_w, whole["cell"] % scene.cell_w
            inside = (cz >= row0) & (cz < row0 + rows) & (cx >= col0) & (cx < col0 + cols)
            assert part["segments"].tobytes() == whole["segments"][inside].tobytes()
            assert np.array_equal(part["level_index"], whole["level_index"][inside])
        half = scene.run(levels, capacity=whole["total"] // 2)
        assert half["total"] == whole["total"] and half["segments"].tobytes() == whole["segments"][:whole["total"] // 2].tobytes()
        prims = scene.run(levels, rgba=(0.1, 0.2, 0.3, 0.8))["prims"]
        want = np.zeros((whole["total"], 20), f32)
        want[:, 0:4], want[:, 4:6] = whole["segments"], whole["segments"][:, 2:4]
        want[:, 6:18] = np.tile(np.array([0.1, 0.2, 0.3, 0.8], f32), 3)
        assert prims.tobytes() == want.view(np.uint32).tobytes(), "v = (a, b, b), one colour, feature 0, reserved 0"
    finally:
        scene.close()


def _end_keys(segments):
    s = np.where(segments == 0.0, f32(0.0), segments).view(np.uint32).reshape(-1, 2, 2).astype(np.uint64)
    return (s[:, :, 0] << np.uint64(32)) | s[:, :, 1]


@pytest.mark.parametrize("shape,spacing", [cases.SHAPES[4], cases.SHAPES[6]], ids=["33x33", "65x63"])
def test_neighbouring_cells_share_their_crossings_bit_for_bit(harness, shape, spacing):
    scene = _scene(harness, shape, spacing, 2.5)
    try:
        levels = cases.level_lists(scene.heights, steep=False)["interval"]
        levels = levels[~np.isin(levels, scene.heights)]
        assert len(levels) >= 8
        for region in cases.regions(shape).values():
            row0, col0, rows, cols = region
            got = scene.run(levels, region)
            seg, idx = got["segments"], got["level_index"]
            xs = plane_at(scene.origin[0], np.array([col0, col0 + cols]), scene.spacing[0])
            zs = plane_at(scene.origin[1], np.array([row0, row0 + rows]), scene.spacing[1])
            ends = seg.reshape(-1, 2)
            border = np.isin(ends[:, 0], xs) | np.isin(ends[:, 1], zs)
            keys = _end_keys(seg).reshape(-1)
            per_level = np.repeat(idx, 2)
            for k in np.unique(idx):
                sel = (per_level == k) & ~border
                _, counts = np.unique(keys[sel], return_counts=True)
                assert (counts == 2).all(), "an interior crossing is the end of exactly two segments"
    finally:
        scene.close()


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_planar_ramp_has_straight_lines_at_the_analytic_positions(harness):
    rows, cols = 9, 17
    dem = np.tile(np.arange(cols, dtype=f32) * f32(2.0), (rows, 1))  # h = 2 i: 2 m a cell of 5 m
    scene = cases.HostContours(harness, dem, cases.shape_kw(dem, (5.0, 3.0), 1.0))
    try:
        levels = np.array([3.0, 7.5, 20.5], f32)
        got = scene.run(levels)
        assert got["total"] == 3 * (rows - 1), "one segment a row of cells and level"
        seg, idx = got["segments"], got["level_index"]
        x_want = float(scene.origin[0]) + levels[idx].astype(np.float64) / 2.0 * 5.0
        assert np.abs(seg[:, 0] - x_want).max() <= 4.0 * ULP * 40.0 and np.abs(seg[:, 2] - x_want).max() <= 4.0 * ULP * 40.0
        assert np.allclose(np.abs(seg[:, 3] - seg[:, 1]), 3.0), "each spans its cell in z"
        polylines = [p for p in cases_chain(seg, idx)]
        assert len(polylines) == 3 and not any(p["closed"] for p in polylines)
        assert all(abs(ref.polyline_length(p["points"]) - 3.0 * (rows - 1)) < 1e-4 for p in polylines)
    finally:
        scene.close()


def cases_chain(seg, idx):
    from forge3d_amd.session import TerrainSession

    return TerrainSession.chain_contours(seg, idx)


def test_checkerboard_makes_every_cell_a_saddle(harness):
    j, i = np.meshgrid(np.arange(10), np.arange(9), indexing="ij")
    dem = ((i + j) % 2).astype(f32)
    scene = cases.HostContours(harness, dem, cases.shape_kw(dem, None, 1.0))
    try:
        got = scene.run(np.array([0.5], f32), details=True)
        assert got["total"] == 2 * 9 * 8 and set(got["case"].tolist()) == {6, 9}
        _check_against_reference(scene, np.array([0.5], f32), None)
    finally:
        scene.close()


def test_plateau_exactly_at_the_level(harness):
    dem = np.zeros((9, 9), f32)
    dem[3:6, 3:6] = 1.0  # a plateau of 3 x 3 samples
    scene = cases.HostContours(harness, dem, cases.shape_kw(dem, None, 2.5))
    try:
        got, _ = _check_against_reference(scene, np.array([2.5], f32), None)  # the level IS the plateau (1.0 * 2.5)
        # h >= level on the plateau only: its inner cells are case 15, the ring around it carries the line, through the plateau's
        # border samples: every crossing has t == 0 or 1 and lies on a sample
        xs = plane_at(scene.origin[0], np.arange(9), scene.spacing[0])
        zs = plane_at(scene.origin[1], np.arange(9), scene.spacing[1])
        ends = got["segments"].reshape(-1, 2)
        assert got["total"] == 12 and np.isin(ends[:, 0], xs).all() and np.isin(ends[:, 1], zs).all()
        above, _ = _check_against_reference(scene, np.array([2.5000002], f32), None)
        assert above["total"] == 0
    finally:
        scene.close()


@pytest.mark.parametrize("shape,spacing", [((63, 65), (10.0, 10.0)), ((33, 33), (10.0, 7.0))], ids=["65x63 at (10, 10) m", "33x33 at (10, 7) m"])
def test_cone(harness, shape, spacing):
    """h = 400 - r.  Level 367 (radius 33 m, between samples): every crossing is used by exactly two ends, one closed loop,
    within 1 % of 2 pi r -- the acceptance figure of the rule restated here (a condition, not a measurement; the float64
    reference's own polygon is printed beside it).  Level 350 (radius 50 m) passes through lattice samples -- (+-50, 0) on both
    lattices, (0, +-50), (+-30, +-40) and (+-40, +-30) too at 10 m --: crossings coincide in fours and sixes and chains end there."""
    dem = cases.cone(shape, spacing)
    scene = cases.HostContours(harness, dem, cases.shape_kw(dem, spacing, 1.0))
    try:
        for level, radius in ((367.0, 33.0), (350.0, 50.0)):
            half_w, half_h = 0.5 * (shape[1] - 1) * spacing[0], 0.5 * (shape[0] - 1) * spacing[1]
            if radius >= min(half_w, half_h):
                continue
            got, ratio = _check_against_reference(scene, np.array([level], f32), None)
            assert ratio <= TOL
            seg, idx = got["segments"], got["level_index"]
            keys, counts = np.unique(_end_keys(seg).reshape(-1), return_counts=True)
            chains = cases_chain(seg, idx)
            length = sum(ref.polyline_length(p["points"]) for p in chains)
            print(f"cone {shape[1]}x{shape[0]} level {level}: {got['total']} segments, {len(chains)} chains, length {length:.4f} = "
                  f"{100.0 * (length / (2.0 * np.pi * radius) - 1.0):+.3f} % of 2 pi r")
            assert abs(length / (2.0 * np.pi * radius) - 1.0) <= 0.01
            on_sample = np.isin(level, scene.heights)
            if not on_sample:
                assert (counts == 2).all()
                assert len(chains) == 1 and chains[0]["closed"] and np.array_equal(chains[0]["points"][0], chains[0]["points"][-1])
            else:
                assert set(counts.tolist()) <= {2, 4, 6} and (counts > 2).any(), "crossings coincide in fours and sixes on samples"
                many = set(keys[counts > 2].tolist())
                assert len(chains) > 1 and not any(p["closed"] for p in chains)
                for p in chains:
                    k = _end_keys(np.concatenate([p["points"][0], p["points"][-1]])[None, :])[0]
                    assert int(k[0]) in many and int(k[1]) in many, "chains end at the points where more than two ends meet"
    finally:
        scene.close()


# ---- chain_contours on hand-made inputs --------------------------------------------------------------------------------------
def test_chain_contours_on_hand_made_inputs():
    chain = cases_chain
    # an open path given out of order and with a reversed segment
    seg = np.array([[1, 0, 2, 0], [0, 0, 1, 0], [3, 1, 2, 0]], f32)
    (p,) = chain(seg, np.zeros(3, np.uint32))
    assert not p["closed"] and p["level_index"] == 0
    assert p["points"].tolist() in ([[0, 0], [1, 0], [2, 0], [3, 1]], [[3, 1], [2, 0], [1, 0], [0, 0]])
    # a loop: the first point is repeated at the end
    loop = np.array([[0, 0, 1, 0], [1, 0, 1, 1], [0, 1, 1, 1], [0, 1, 0, 0]], f32)
    (p,) = chain(loop, np.full(4, 5, np.uint32))
    assert p["closed"] and p["level_index"] == 5 and len(p["points"]) == 5 and p["points"][0].tolist() == p["points"][-1].tolist()
    # two levels never join, although their ends coincide
    two = chain(np.array([[0, 0, 1, 0], [1, 0, 2, 0]], f32), np.array([0, 1], np.uint32))
    assert [q["level_index"] for q in two] == [0, 1] and all(len(q["points"]) == 2 for q in two)
    # a branching point ends the chains there; a zero-length segment is dropped; -0 is +0
    star = np.array([[0, 0, 1, 1], [1, 1, 2, 0], [1, 1, 1, 2], [1, 2, 1, 3], [1, 1, 1, 1], [-0.0, 0, -1, 0]], f32)
    parts = chain(star, np.zeros(6, np.uint32))
    assert len(parts) == 3 and not any(q["closed"] for q in parts)
    assert sorted(len(q["points"]) for q in parts) == [2, 3, 3]
    assert sum(ref.polyline_length(q["points"]) for q in parts) == pytest.approx(2 * 2 ** 0.5 + 3.0)
    assert chain(np.zeros((0, 4), f32), np.zeros(0, np.uint32)) == []
    with pytest.raises(ValueError, match="2 segments but 1 level indices"):
        chain(np.zeros((2, 4), f32), np.zeros(1, np.uint32))


# ---- the sanitizer run: a stand-alone program, never code loaded into this process ---------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(cases.HARNESS, "contour")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "disagreements: 0" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- the interface -------------------------------------------------------------------------------------------------------------
MEMBERS = {
    "f3d_session_contours_desc": ["struct_size", "flags", "row0", "col0", "rows", "cols", "level_count", "reserved", "levels", "segments", "level_index",
                                  "capacity", "total"],
    "f3d_session_paint_contours_desc": ["struct_size", "flags", "row0", "col0", "rows", "cols", "level_count", "reserved", "levels", "total", "rgba",
                                        "half_width", "opacity", "aim"],
}


def _header_members(header, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            out += [re.sub(r"\[\d+\]", "", first.split()[-1].lstrip("*"))] + [m.strip().lstrip("*") for m in more]
    return out


def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header and _native.ABI_VERSION == 6, "the contour entry points are additive: no ABI version bump"
    structs = {"f3d_session_contours_desc": _native.ContoursDesc, "f3d_session_paint_contours_desc": _native.PaintContoursDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "f3d_terrain_pt.h"', "int main(void) {"]
    for name, ctype in structs.items():
        assert _header_members(header, name) == [n for n, _ in ctype._fields_] == MEMBERS[name]
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {m}));' for m in MEMBERS[name]]
        lines.append('  printf("\\n");')
    lines.append("  return 0; }")
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "layout.c"
        c.write_text("\n".join(lines))
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "layout")], check=True)
        rows = subprocess.run([str(Path(tmp) / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    for row, (name, ctype) in zip(rows, structs.items()):
        want = [C.sizeof(ctype)] + [getattr(ctype, m).offset for m in MEMBERS[name]]
        assert [int(v) for v in row.split()] == want, name
    assert C.sizeof(_native.ContoursDesc) == 72 == harness.contour_desc_size(0)
    assert C.sizeof(_native.PaintContoursDesc) == 72 + C.sizeof(_native.ReaimDesc) == harness.contour_desc_size(1)
    for fn, desc in (("f3d_session_contours", "f3d_session_contours_desc"), ("f3d_session_paint_contours", "f3d_session_paint_contours_desc")):
        assert re.search(rf"int {fn}\(f3d_session \*session, const {desc} \*desc, char \*err, size_t errlen\);", header)
        entry = [e for e in _native.ABI if e[0] == fn]
        assert len(entry) == 1 and entry[0][1] is C.c_int
    assert re.search(r"#define F3D_CONTOUR_DEVICE_POINTERS 4u", header) and _native.CONTOUR_DEVICE_POINTERS == 4 == _native.RASTER_DEVICE_POINTERS
    assert re.search(r"#define F3D_CONTOUR_MAX_LEVELS 65536u", header) and _native.CONTOUR_MAX_LEVELS == 65536
    assert "csrc/f3d_contour.h" in header, "the ABI header refers to the contract"
    assert "f3d_contour.hip" in _native.HIP_SOURCES


def test_integration_guide_has_the_structs_and_the_externs():
    text = (ROOT / "INTEGRATION.md").read_text()
    for rust, cname in (("F3dSessionContoursDesc", "f3d_session_contours_desc"), ("F3dSessionPaintContoursDesc", "f3d_session_paint_contours_desc")):
        body = re.search(rf"pub struct {rust} \{{(.*?)\n\}}", text, re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == MEMBERS[cname]
        types = {k: v.strip() for k, v in re.findall(r"pub (\w+): ([^,]+),", body)}
        assert all(types[n] == "u32" for n in MEMBERS[cname][:8]) and types["levels"] == "*const f32" and types["total"] == "*mut u64"
        fn = cname[:-5]
        assert re.search(rf"pub fn {fn}\(session: \*mut F3dSession, desc: \*const {rust}, err: \*mut c_char, errlen: usize\) -> c_int;", text)
    assert "pub capacity: u64" in text and "pub rgba: [f32; 4]" in text and "pub aim: F3dSessionReaimDesc" in text


def test_both_entry_points_answer_status_4_without_a_device():
    """In a process without a HIP device both entry points answer F3D_STATUS_DEVICE before any other check -- whatever session
    and descriptor they are handed -- and write nothing.  (With a device the probe passes and the null session is the first
    refusal, status 1; the refusals on a live session are tests/test_gpu_contour.py's.)"""
    from forge3d_amd import _native

    L = _native.lib()
    have_device = _native.device_count() > 0
    total = C.c_uint64(7)
    q = _native.ContoursDesc()
    q.struct_size = C.sizeof(q)
    q.total = C.addressof(total)
    p = _native.PaintContoursDesc()
    p.struct_size = C.sizeof(p)
    p.total = C.addressof(total)
    for call, own in ((L.f3d_session_contours, q), (L.f3d_session_paint_contours, p)):
        for desc in (own, None):  # (its descriptor, or none: the probe comes first)
            err = C.create_string_buffer(256)
            rc = call(None, None if desc is None else C.byref(desc), err, len(err))
            if have_device:
                assert rc == _native.STATUS_VALUE and err.value == b"null session handle"
            else:
                assert rc == _native.STATUS_DEVICE == 4 and err.value == b"no HIP device available: libf3dhip has no CPU fallback"
    assert total.value == 7
    if not have_device:
        from forge3d_amd.session import TerrainSession

        dem = cases.shaped_dem((9, 9))
        with pytest.raises(RuntimeError, match=r"\[Device\].*no CPU fallback"):
            TerrainSession(dem, *cases.SIZE, **cases.shape_kw(dem))


def _bare_session(dem_shape=(9, 9), bottom=0.0, top=100.0):
    from forge3d_amd.session import TerrainSession

    s = TerrainSession.__new__(TerrainSession)
    s.dem_shape = dem_shape
    s._terrain_bottom, s._terrain_top = bottom, top
    s._handle = None
    return s


def test_wrapper_methods_and_argument_checks(monkeypatch):
    import inspect

    from forge3d_amd.session import TerrainSession

    p = inspect.signature(TerrainSession.contours).parameters
    assert list(p) == ["self", "levels", "interval", "base", "region", "chain", "out"] and p["levels"].default is None
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("interval", "base", "region", "chain", "out"))
    q = inspect.signature(TerrainSession.paint_contours).parameters
    assert list(q)[:2] == ["self", "levels"] and q["rgba"].default == (0.0, 0.0, 0.0, 0.8) and q["width"].default == 1.0 and q["opacity"].default == 1.0
    assert q["rearmable"].kind is inspect.Parameter.VAR_KEYWORD and q["camera"].default is None and q["region"].default is None
    assert isinstance(inspect.getattr_static(TerrainSession, "chain_contours"), staticmethod)
    _no_device(monkeypatch)
    s = _bare_session()
    lv = s.contour_levels(25.0)
    assert lv.dtype == np.float32 and lv.tolist() == [0.0, 25.0, 50.0, 75.0, 100.0]
    assert s.contour_levels(40.0, base=10.0).tolist() == [-30.0, 10.0, 50.0, 90.0, 130.0], "the levels contain the height range"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="interval must be finite and > 0"):
            s.contour_levels(bad)
    with pytest.raises(ValueError, match="at most 65536"):
        s.contour_levels(1e-4)
    for call in (s.contours, s.paint_contours):
        with pytest.raises(ValueError, match="either levels or interval"):
            call()
        with pytest.raises(ValueError, match="either levels or interval"):
            call([1.0], interval=2.0)
        with pytest.raises(ValueError, match="strictly ascending"):
            call([1.0, 1.0])
        with pytest.raises(ValueError, match="strictly ascending"):
            call([1.0, float("nan")])
        with pytest.raises(ValueError, match="levels is empty"):
            call([])
        with pytest.raises(ValueError, match="at most 65536 levels"):
            call(np.arange(65537, dtype=np.float32))
        with pytest.raises(ValueError, match="must not be negative"):
            call([1.0], region=(0, -1, 2, 2))
    with pytest.raises(ValueError, match="chain=True joins segments on the host"):
        s.contours([1.0], chain=True, out=(None, None))
    with pytest.raises(TypeError, match="unexpected keyword argument 'spp'"):
        s.paint_contours([1.0], spp=2)
    with pytest.raises(ValueError, match="one colour of 3 or 4 numbers"):
        s.paint_contours([1.0], rgba=(0.0, 1.0))
    with pytest.raises(ValueError, match="width must be finite and >= 0"):
        s.paint_contours([1.0], width=-1.0)
    with pytest.raises(ValueError, match=re.escape("opacity must lie in [0, 1]")):
        s.paint_contours([1.0], opacity=1.5)


# ---- what contours() and streams(), paint_contours() and paint_streams() share in the wrapper: every text in full ------------
def device_tensor(shape, dtype, contiguous=True):
    """What the wrapper's checks see of a tensor on the session's device, without a device."""
    import torch

    members = {"__module__": "torch", "is_cuda": True, "ndim": len(shape), "shape": tuple(shape), "dtype": getattr(torch, dtype),
               "is_contiguous": lambda self: contiguous, "data_ptr": lambda self: 256, "numel": lambda self: int(np.prod(shape))}
    return type("Tensor", (), members)()


class UntouchedLibrary:
    """The session's library for a call that must be refused before it: an entry may be looked up, not called."""
    def __getattr__(self, name):
        def entry(*a):
            raise AssertionError("the device was touched")
        return entry


def refused(text, call, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        call(*args, **kw)


def record_outputs_refusals(call, second):
    """``call(out)``: contours() or streams() with their own arguments in place."""
    seg_text = f"out=(segments, {second}): segments must be a contiguous float32 tensor (C, 4) on the session's device"
    second_text = f"out=(segments, {second}): {second} must be a contiguous int32 tensor (C,) on the session's device, or None"
    good = device_tensor((6, 4), "float32")
    for seg in (np.zeros((6, 4), np.float32), [[0.0] * 4] * 6, device_tensor((6, 3), "float32"), device_tensor((6, 4), "float64"),
                device_tensor((6, 4), "float32", contiguous=False), device_tensor((24,), "float32")):
        refused(seg_text, call, (seg, None))
        refused(seg_text, call, (seg, np.zeros(5)))  # (the segments' fault wins)
    for word in (np.zeros(6, np.uint32), device_tensor((5,), "int32"), device_tensor((7,), "int32"), device_tensor((6,), "uint8"),
                 device_tensor((6,), "int64"), device_tensor((6, 1), "int32"), device_tensor((6,), "int32", contiguous=False)):
        refused(second_text, call, (good, word))


def stroke_refusals(call):
    """``call(**stroke)``: paint_contours() or paint_streams() with their own arguments in place."""
    refused("rgba must be one colour of 3 or 4 numbers, got (2,)", call, rgba=(0.0, 1.0))
    refused("rgba must be one colour of 3 or 4 numbers, got (5,)", call, rgba=(0.0, 1.0, 0.0, 1.0, 0.5))
    refused("rgba must be one colour of 3 or 4 numbers, got (2,)", call, rgba=(0.0, 1.0), width=-1.0)  # (the colour's fault wins)
    refused("width must be finite and >= 0 metres, got -1.0", call, width=-1.0)
    refused("width must be finite and >= 0 metres, got nan", call, width=float("nan"))
    refused("width must be finite and >= 0 metres, got -1.0", call, width=-1.0, opacity=1.5)  # (the width's fault wins)
    refused("opacity must lie in [0, 1], got 1.5", call, opacity=1.5)


def test_shared_refusals_of_the_record_outputs_and_the_stroke_in_the_contours_words(monkeypatch):
    _no_device(monkeypatch)
    s = _bare_session()
    s._lib = UntouchedLibrary()
    record_outputs_refusals(lambda out: s.contours([1.0], out=out), "level_index")
    stroke_refusals(lambda **stroke: s.paint_contours([1.0], **stroke))
