"""Drainage through depressions (f3d_session_fill, F3D_DRAINAGE_FILL on the drainage entries), the parts that need no GPU.

The lane and tile bodies of the fill kernels (csrc/f3d_fill.h) compiled for the host (tests/fill_host) -- the tile body at the
device's edge AND at an edge of 8, the tiles of a round in index order AND in a shuffled one -- against tests/fill_reference.py,
an independent statement of the contract (a priority-flood with a heap, a BFS per plateau, the direction rule sample by sample,
accumulation in descending (W, T)) that knows nothing of tiles, rounds or doubling.  EVERY COMPARISON IS EXACT (bits).

* DEMs: the 21 named cases of the drainage tests, a 5x5 pit, a nested depression on 9x9 with two spill levels, a random relief
  of 65x130 at (10, 7) m, and the walled serpentine -- a channel that ASCENDS to its end inside a frame with one gap -- at 35x35
  and at (2 TILE + 3)^2, three by three tiles of the device's edge with partial ones;
* W, depth, T, direction, accumulation, basin, sinks and longest equal the reference and each other across both edges and
  both orders; the fixed-point identity on every non-outlet; W >= z, W == z on outlets; every sink an outlet; the sinks'
  accumulations sum to w * h; every receiver has a smaller (W, T); rounds == floor(log2 longest) + 1; a region is the whole
  DEM's slice; with the fill off the harness returns tests/drainage_host's bits;
* known answers: the flat, the bowl, the pit, the 35x35 walled serpentine;
* stream records over the filled routing equal drainage_reference.streams over the reference's;
* a stand-alone driver (its own main) of the same bodies under -fsanitize=address,undefined, run once on the serpentine;
* the header, the ctypes table, the descriptor's layout, INTEGRATION.md's struct; the wrapper's methods and checks; status 4
  without a device.
"""
from __future__ import annotations

import ctypes as C
import inspect
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import drainage_cases as cases
import drainage_reference as ref
import fill_cases
import fill_reference as fref
from emul import emul
from test_session_contour_host import _header_members
from test_session_drainage_host import _bare_session
from test_session_rearm_host import _no_device

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
FILL_PLANES = ("filled", "depth", "flat_distance")
DRAIN_PLANES = ("direction", "accumulation", "basin")
SEED = 3


@pytest.fixture(scope="module")
def harness():
    return fill_cases.build_harness()


@pytest.fixture(scope="module")
def drainage_harness():
    return cases.build_harness()


def _tile():
    return int(re.search(r"constexpr uint32_t kFillTile = (\d+)u;", (ROOT / "forge3d_amd" / "csrc" / "f3d_fill.h").read_text()).group(1))


TILE = _tile()
CASES = dict(cases.named_cases())
CASES.update(fill_cases.extra_cases(TILE))
BIG = f"walled serpentine {2 * TILE + 3}"


@pytest.fixture(scope="module")
def routed(harness):
    """name -> the scene's values, the reference's answer and the host body's for (edge, seed) in both edges and both orders:
    computed once, left unchanged."""
    assert int(harness.fill_tile_edge()) == TILE
    out = {}
    for name, (dem, spacing, e) in CASES.items():
        scene = fill_cases.HostFill(harness, dem, cases.shape_kw(dem, spacing, e))
        try:
            got = {(edge, seed): (scene.fill(edge=edge, seed=seed), scene.drainage(edge=edge, seed=seed)) for edge in (fill_cases.SMALL, TILE) for seed in (0, SEED)}
            out[name] = {"heights": scene.heights, "origin": scene.origin, "spacing": scene.spacing, "dem": scene.dem, "got": got,
                         "want": fref.route(scene.heights, scene.spacing), "plain": scene.drainage(edge=0)}
        finally:
            scene.close()
    return out


def _scene(harness, name):
    dem, spacing, e = CASES[name]
    return fill_cases.HostFill(harness, dem, cases.shape_kw(dem, spacing, e))


def test_the_cases_are_the_ones_the_contract_names():
    assert len(cases.named_cases()) == 21 and len(CASES) == 26
    assert CASES["pit"][0].shape == (5, 5) and CASES["nested"][0].shape == (9, 9) and CASES["relief 65x130"][0].shape == (65, 130)
    assert CASES["relief 65x130"][1] == (10.0, 7.0)
    assert CASES["walled serpentine 35x35"][0].shape == (35, 35) and CASES[BIG][0].shape == (2 * TILE + 3, 2 * TILE + 3)


@pytest.mark.parametrize("name", list(CASES))
def test_host_body_against_the_reference(harness, routed, name):
    r = routed[name]
    want, z = r["want"], (r["heights"] + f32(0.0)).astype(f32)
    rows, cols = z.shape
    outlet = fref.outlets(z.shape)
    for (edge, seed), (fill, drain) in r["got"].items():
        what = f"{name}, edge {edge}, seed {seed}"
        for plane in FILL_PLANES:
            assert fill[plane].dtype == want[plane].dtype and fill[plane].tobytes() == want[plane].tobytes(), (what, plane)
        for plane in DRAIN_PLANES:
            assert drain[plane].dtype == want[plane].dtype and np.array_equal(drain[plane], want[plane]), (what, plane)
        assert (fill["filled_samples"], fill["largest_flat_distance"]) == (want["filled_samples"], want["largest_flat_distance"]), what
        assert (drain["sinks"], drain["longest"]) == (want["sinks"], want["longest"]), what
        assert drain["rounds"] == ref.rounds(want["longest"]) == (0 if drain["longest"] == 0 else int(np.floor(np.log2(drain["longest"]))) + 1), what
        assert fill["fill_rounds"] >= 1 and (fill["flat_rounds"] >= 1) == bool((want["flat_distance"] > 0).any()), what
    # (the four runs equal the reference, hence each other; the properties are checked on one of them)
    fill, drain = r["got"][(TILE, 0)]
    W, T = fill["filled"], fill["flat_distance"]
    assert (W >= z).all() and np.array_equal(W[outlet], z[outlet]) and fill["depth"].tobytes() == (W - z).astype(f32).tobytes()
    low = np.full(z.shape, np.inf, f32)
    for dj, di in ref.STEPS:
        j0, j1, i0, i1 = max(0, -dj), min(rows, rows - dj), max(0, -di), min(cols, cols - di)
        low[j0:j1, i0:i1] = np.minimum(low[j0:j1, i0:i1], W[j0 + dj:j1 + dj, i0 + di:i1 + di])
    assert np.array_equal(W[~outlet], np.maximum(z, low)[~outlet]), "the fixed-point identity on every non-outlet"
    assert (T != fref.FAR).all()
    sink = drain["direction"] == ref.SINK
    assert outlet[sink].all(), "every sink is an outlet"
    assert int(drain["accumulation"][sink].astype(np.int64).sum()) == z.size, "the sinks' accumulations sum to w * h"
    recv, flat_sink = ref.receivers(drain["direction"]), sink.reshape(-1)
    Wf, Tf = W.reshape(-1), T.reshape(-1)
    lower = (Wf[recv] < Wf) | ((Wf[recv] == Wf) & (Tf[recv] < Tf))
    assert lower[~flat_sink].all(), "every receiver has a smaller (W, T)"
    assert np.array_equal(drain["basin"].reshape(-1)[flat_sink], np.nonzero(flat_sink)[0]), "a sink labels itself"
    scene = _scene(harness, name)
    try:
        for rname, region in cases.regions(z.shape).items():
            row0, col0, nr, nc = region
            cut = (slice(row0, row0 + nr), slice(col0, col0 + nc))
            part_fill, part = scene.fill(region, edge=fill_cases.SMALL, seed=SEED), scene.drainage(region, edge=fill_cases.SMALL, seed=SEED)
            for plane in FILL_PLANES:
                assert part_fill[plane].tobytes() == np.ascontiguousarray(want[plane][cut]).tobytes(), (rname, plane)
            for plane in DRAIN_PLANES:
                assert np.array_equal(part[plane], want[plane][cut]), (rname, plane)
            assert (part["sinks"], part["rounds"], part["longest"]) == (drain["sinks"], drain["rounds"], drain["longest"]), "the whole DEM is routed"
            assert part_fill["filled_samples"] == fill["filled_samples"]
    finally:
        scene.close()


@pytest.mark.parametrize("name", list(cases.named_cases()))
def test_with_the_fill_off_the_harness_returns_the_drainage_harness_bits(drainage_harness, routed, name):
    dem, spacing, e = CASES[name]
    scene = cases.HostDrainage(drainage_harness, dem, cases.shape_kw(dem, spacing, e))
    try:
        want, got = scene.run(), routed[name]["plain"]
        for plane in DRAIN_PLANES:
            assert np.array_equal(got[plane], want[plane]), plane
        assert (got["sinks"], got["rounds"], got["longest"]) == (want["sinks"], want["rounds"], want["longest"])
    finally:
        scene.close()


def test_known_answers(routed):
    def both(name):
        return routed[name]["got"][(TILE, 0)]

    fill, drain = both("flat")
    assert fill["filled_samples"] == 0 and drain["sinks"] == 34 and fill["largest_flat_distance"] == 4 and drain["longest"] == 4
    j, i = np.meshgrid(np.arange(9), np.arange(10), indexing="ij")
    assert np.array_equal(fill["flat_distance"], np.minimum(np.minimum(j, 8 - j), np.minimum(i, 9 - i))), "the distance to the border in king's moves"
    fill, drain = both("bowl")
    assert fill["filled_samples"] == 45 and drain["sinks"] == 4
    fill, drain = both("pit")
    assert fill["filled_samples"] == 1 and drain["sinks"] == 1 and int(drain["accumulation"].max()) == 25
    assert drain["accumulation"][drain["direction"] == ref.SINK].tolist() == [25]
    fill, drain = both("nested")
    assert len(np.unique(fill["filled"][fill["depth"] > 0])) == 2, "two spill levels"
    fill, drain = both("walled serpentine 35x35")
    assert (fill["filled_samples"], fill["largest_flat_distance"], drain["sinks"], int(drain["accumulation"].max()), drain["longest"]) == (577, 544, 1, 1225, 545)
    fill, drain = both(BIG)
    assert drain["sinks"] == 1 and int(drain["accumulation"].max()) == (2 * TILE + 3) ** 2
    assert routed[BIG]["plain"]["sinks"] == 1 and routed["relief 65x130"]["plain"]["sinks"] > 10 * routed["relief 65x130"]["want"]["sinks"]


@pytest.mark.parametrize("name", ["5x3 x1.0", "65x63 x2.5", "flat", "nested", "relief 65x130", "walled serpentine 35x35"])
def test_stream_records_over_the_filled_routing(harness, routed, name):
    r = routed[name]
    scene = _scene(harness, name)
    try:
        top = int(r["want"]["accumulation"].max())
        for threshold in sorted({1, 2, max(2, top // 8), top, top + 1}):
            for rname, region in cases.regions(r["dem"].shape).items():
                want = ref.streams(r["want"], r["origin"], r["spacing"], threshold, region)
                for edge, seed in ((TILE, 0), (fill_cases.SMALL, SEED)):
                    got = scene.streams(threshold, region, edge=edge, seed=seed)
                    assert got["total"] == len(want["segments"]), (threshold, rname)
                    assert got["segments"].tobytes() == want["segments"].tobytes() and np.array_equal(got["accumulation"], want["accumulation"])
        n = scene.streams(1)["total"]
        assert n == r["dem"].size - r["want"]["sinks"], "threshold 1: every sample that is no sink"
        painted = scene.streams(1, rgba=(0.1, 0.3, 0.8, 1.0))
        want = np.zeros((n, 20), f32)
        want[:, 0:4], want[:, 4:6] = painted["segments"], painted["segments"][:, 2:4]
        want[:, 6:18] = np.tile(np.array([0.1, 0.3, 0.8, 1.0], f32), 3)
        assert painted["prims"].tobytes() == want.view(np.uint32).tobytes(), "the paint form's records"
    finally:
        scene.close()


# ---- the sanitizer run: a stand-alone program, never code loaded into this process ---------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(fill_cases.HARNESS, "fill_host")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "577 filled, largest T 544, 1 sinks, longest 545" in run.stdout and "disagreements: 0" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- the interface -------------------------------------------------------------------------------------------------------------
MEMBERS = ["struct_size", "flags", "row0", "col0", "rows", "cols", "filled", "depth", "flat_distance", "stats", "ms", "reserved"]


def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header and _native.ABI_VERSION == 6, "the fill is additive: no ABI version bump"
    assert _header_members(header, "f3d_session_fill_desc") == [n for n, _ in _native.FillDesc._fields_] == MEMBERS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "f3d_terrain_pt.h"', "int main(void) {", '  printf("%zu", sizeof(f3d_session_fill_desc));']
    lines += [f'  printf(" %zu", offsetof(f3d_session_fill_desc, {m}));' for m in MEMBERS]
    lines.append("  return 0; }")
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "layout.c"
        c.write_text("\n".join(lines))
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "layout")], check=True)
        row = subprocess.run([str(Path(tmp) / "layout")], capture_output=True, text=True, check=True).stdout
    assert [int(v) for v in row.split()] == [C.sizeof(_native.FillDesc)] + [getattr(_native.FillDesc, m).offset for m in MEMBERS]
    assert C.sizeof(_native.FillDesc) == 72 == harness.fill_desc_size()
    assert re.search(r"int f3d_session_fill\(f3d_session \*session, const f3d_session_fill_desc \*desc, char \*err, size_t errlen\);", header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_fill"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for define, value in (("F3D_DRAINAGE_FILL 8u", _native.DRAINAGE_FILL), ("F3D_STREAMS_FILL 8u", _native.STREAMS_FILL)):
        assert f"#define {define}" in header and value == 8
    assert "#define F3D_FILL_DEVICE_POINTERS 4u" in header and _native.FILL_DEVICE_POINTERS == 4 == _native.RASTER_DEVICE_POINTERS
    assert "#define F3D_DRAINAGE_DEVICE_POINTERS 4u" in header and "#define F3D_DRAINAGE_SINK 8u" in header, "what was there stays"
    assert "csrc/f3d_fill.h" in header, "the ABI header refers to the contract"
    assert "f3d_fill.hip" in _native.HIP_SOURCES
    host = (ROOT / "forge3d_amd" / "csrc" / "f3d_host_drainage.h").read_text()
    assert "kDrainBytesPerSample = 21u" in host and "kDrainFilledBytesPerSample = 33u" in host
    assert "33" in header[header.index("21 bytes a DEM sample"):][:40] and "33 bytes" in (ROOT / "DESIGN.md").read_text()


def test_integration_guide_has_the_struct_and_the_extern():
    text = (ROOT / "INTEGRATION.md").read_text()
    body = re.search(r"pub struct F3dSessionFillDesc \{(.*?)\n\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == MEMBERS
    types = {k: v.strip() for k, v in re.findall(r"pub (\w+): ([^,]+),", body)}
    assert all(types[n] == "u32" for n in MEMBERS[:6]) and types["reserved"] == "u32"
    assert (types["filled"], types["depth"], types["flat_distance"], types["stats"], types["ms"]) == ("*mut f32", "*mut f32", "*mut u32", "*mut u32", "*mut f64")
    assert re.search(r"pub fn f3d_session_fill\(session: \*mut F3dSession, desc: \*const F3dSessionFillDesc, err: \*mut c_char, errlen: usize\) -> c_int;", text)
    assert "F3D_DRAINAGE_FILL" in text


def test_the_entry_point_answers_status_4_without_a_device():
    from forge3d_amd import _native

    L = _native.lib()
    have_device = _native.device_count() > 0
    stats = (C.c_uint32 * 4)(7, 7, 7, 7)
    q = _native.FillDesc()
    q.struct_size, q.stats = C.sizeof(q), C.addressof(stats)
    for desc in (q, None):
        err = C.create_string_buffer(256)
        rc = L.f3d_session_fill(None, None if desc is None else C.byref(desc), err, len(err))
        if have_device:
            assert rc == _native.STATUS_VALUE and err.value == b"null session handle"
        else:
            assert rc == _native.STATUS_DEVICE == 4 and err.value == b"no HIP device available: libf3dhip has no CPU fallback"
    assert list(stats) == [7, 7, 7, 7]
    # the three drainage entries with the FILL flag: the probe still comes first
    total = C.c_uint64(7)
    d = _native.DrainageDesc()
    d.struct_size, d.flags, d.stats = C.sizeof(d), _native.DRAINAGE_FILL, C.addressof(stats)
    s = _native.StreamsDesc()
    s.struct_size, s.flags, s.threshold, s.total = C.sizeof(s), _native.STREAMS_FILL, 1, C.addressof(total)
    p = _native.PaintStreamsDesc()
    p.struct_size, p.flags, p.threshold, p.total = C.sizeof(p), _native.STREAMS_FILL, 1, C.addressof(total)
    for call, desc in ((L.f3d_session_drainage, d), (L.f3d_session_streams, s), (L.f3d_session_paint_streams, p)):
        err = C.create_string_buffer(256)
        assert call(None, C.byref(desc), err, len(err)) == (_native.STATUS_VALUE if have_device else _native.STATUS_DEVICE)
    assert total.value == 7 and list(stats) == [7, 7, 7, 7]


def test_wrapper_methods_and_argument_checks(monkeypatch):
    from forge3d_amd.session import FilledRouting, TerrainSession
    from forge3d_amd.viewer import ViewerError, ViewerHandle

    p = inspect.signature(TerrainSession.fill).parameters
    assert list(p) == ["self", "region", "filled", "depth", "flat_distance", "out"] and p["region"].default is None
    assert (p["filled"].default, p["depth"].default, p["flat_distance"].default, p["out"].default) == (True, False, False, None)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("filled", "depth", "flat_distance", "out"))
    for thin in ("filled_heights", "lake_depth"):
        assert list(inspect.signature(getattr(TerrainSession, thin)).parameters) == ["self", "region"]
    assert inspect.signature(TerrainSession.paint_streams).parameters["fill"].default is False
    assert inspect.signature(ViewerHandle.enable_streams).parameters["fill"].default is False
    # the filled view takes what the session's own calls take (but wait=, which they refuse anyway)
    for name in ("drainage", "flow_directions", "flow_accumulation", "basins", "streams"):
        mine, theirs = inspect.signature(getattr(FilledRouting, name)).parameters, inspect.signature(getattr(TerrainSession, name)).parameters
        assert [n for n in theirs if n != "wait"] == list(mine) and all(mine[n].default == theirs[n].default and mine[n].kind == theirs[n].kind for n in mine), name
    _no_device(monkeypatch)
    s = _bare_session()
    assert isinstance(s.filled, FilledRouting)
    with pytest.raises(ValueError, match="must not be negative"):
        s.fill((0, -1, 2, 2))
    with pytest.raises(ValueError, match="out must be None, 'device' or a dict"):
        s.fill(out="host")
    with pytest.raises(ValueError, match="out must be None, 'device' or a dict"):
        s.fill(out={"direction": None})
    with pytest.raises(ValueError, match="must not be negative"):
        s.filled.drainage((0, -1, 2, 2))
    for call in (s.filled.streams, s.filled.paint_streams, lambda t: s.paint_streams(t, fill=True)):
        with pytest.raises(ValueError, match="threshold is an accumulation"):
            call(0)
    with pytest.raises(ValueError, match="segments must be a contiguous float32 tensor"):
        s.filled.streams(5, out=(np.zeros((4, 4), f32), None))
    with pytest.raises(TypeError, match="unexpected keyword argument 'spp'"):
        s.filled.paint_streams(5, spp=2)
    handle = ViewerHandle.__new__(ViewerHandle)
    handle._revision = 0
    handle.enable_streams(50, fill=True)
    assert handle._streams["fill"] is True and handle._revision == 1
    handle.enable_streams(50)
    assert handle._streams["fill"] is False
    with pytest.raises(ViewerError):
        handle.enable_streams(0, fill=True)


def test_shared_refusals_of_the_planes_in_the_fills_words(monkeypatch):
    from test_session_drainage_host import planes_refusals

    _no_device(monkeypatch)
    s = _bare_session((7, 12))
    # (filled=False: a plane that is wanted and not given is allocated on the way, on a device)
    planes_refusals(lambda out: s.fill(filled=False, out=out), FILL_PLANES, ("float32", "float32", "int32"), (7, 12))
    planes_refusals(lambda out: s.fill((1, 2, 3, 4), filled=False, out=out), FILL_PLANES, ("float32", "float32", "int32"), (3, 4))
