"""Drainage on a live terrain session (f3d_session_drainage, f3d_session_streams, f3d_session_paint_streams), the parts that
need no GPU.

The lane bodies of the drainage kernels (csrc/f3d_drainage.h) compiled for the host (tests/drainage_host) and run over whole
64-lane waves -- the direction pass by tiles, the doubling rounds as Jacobi sweeps, count, scan, emit -- against
tests/drainage_reference.py, an independent NumPy statement of the contract that visits samples in descending height and
knows nothing of waves, tiles or doubling.

* DEMs: the contour tests' 2x2, 5x3, 9x9, 10x9, 33x33 at (10, 7) m, 64x64 and 65x63 at exaggerations 1 and 2.5 (a partial tile,
  more than one wave, an anisotropic diagonal, a row length that is no multiple of 64), and known answers: a planar ramp, a
  bowl, the cone h = 400 - r, a flat, a plateau with a tie, and a serpentine channel on 33x33 (one sink, accumulation 1089,
  longest path 544, 10 rounds);
* directions, accumulation, basins, sinks, rounds and longest equal the reference EXACTLY, for every case and region;
  rounds == floor(log2(longest)) + 1, or 0; the sinks' accumulations sum to w * h; a receiver is strictly lower;
* stream records, counts and order are exact; coordinates are plane_at's bits; a region is the whole DEM's filter;
* the float64 check: the chosen neighbour's float64 slope is at least (1 - 8 x 2^-24) times the largest float64 slope -- DERIVED:
  each f32 slope carries at most four roundings of relative size 2^-24 (the drop, the diagonal's sum and its sqrt, the
  quotient; the products under the sqrt are absorbed by its halving), and the check compares two of them.  No sample is left
  out.  On these inputs the f32 and f64 choices coincide everywhere, which is asserted too, with the count printed;
* a stand-alone driver (its own main) of the same lane bodies built with -fsanitize=address,undefined and run once;
* the header, the ctypes table, the descriptors' layout and INTEGRATION.md's structs; the wrapper's methods and checks.
The refusals of the entry points need a session, i.e. a device: tests/test_gpu_drainage.py.
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import drainage_cases as cases
import drainage_reference as ref
from emul import emul
from test_session_contour_host import _header_members
from test_session_rearm_host import _no_device

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
ULP = 2.0 ** -24
CASES = cases.named_cases()
PROXIES = [n for n in CASES if " x" in n]  # the shaped DEMs at both exaggerations


@pytest.fixture(scope="module")
def harness():
    return cases.build_harness()


@pytest.fixture(scope="module")
def routed(harness):
    """name -> (scene values, the host body's whole-DEM answer, the reference's): computed once, left unchanged."""
    out = {}
    for name, (dem, spacing, e) in CASES.items():
        scene = cases.HostDrainage(harness, dem, cases.shape_kw(dem, spacing, e))
        try:
            got = scene.run()
            want = ref.route(scene.heights, scene.spacing)
            out[name] = {"heights": scene.heights, "origin": scene.origin, "spacing": scene.spacing, "dem": scene.dem, "exaggeration": e,
                         "got": got, "want": want}
        finally:
            scene.close()
    return out


def _scene(harness, name):
    dem, spacing, e = CASES[name]
    return cases.HostDrainage(harness, dem, cases.shape_kw(dem, spacing, e))


@pytest.mark.parametrize("name", list(CASES))
def test_host_body_against_the_reference(harness, routed, name):
    r = routed[name]
    got, want = r["got"], r["want"]
    assert np.array_equal(r["heights"], ref.session_heights(r["dem"], r["exaggeration"])), "the leaf table holds f32(h * exaggeration)"
    for plane in ("direction", "accumulation", "basin"):
        assert got[plane].dtype == want[plane].dtype and np.array_equal(got[plane], want[plane]), plane
    assert (got["sinks"], got["longest"]) == (want["sinks"], want["longest"])
    assert got["rounds"] == ref.rounds(want["longest"]) == (0 if got["longest"] == 0 else int(np.floor(np.log2(got["longest"]))) + 1)
    sink = got["direction"] == ref.SINK
    assert int(got["accumulation"][sink].astype(np.int64).sum()) == sink.size, "the sinks' accumulations sum to w * h"
    flat = r["heights"].reshape(-1)
    recv = ref.receivers(got["direction"])
    assert (flat[recv[~sink.reshape(-1)]] < flat[~sink.reshape(-1)]).all(), "a receiver is strictly lower"
    assert np.array_equal(got["basin"].reshape(-1)[sink.reshape(-1)], np.nonzero(sink.reshape(-1))[0]), "a sink labels itself"
    scene = _scene(harness, name)
    try:
        for rname, region in cases.regions(r["dem"].shape).items():
            row0, col0, rows, cols = region
            part = scene.run(region)
            for plane in ("direction", "accumulation", "basin"):
                assert np.array_equal(part[plane], want[plane][row0:row0 + rows, col0:col0 + cols]), (rname, plane)
            assert (part["sinks"], part["rounds"], part["longest"]) == (got["sinks"], got["rounds"], got["longest"]), "the whole DEM is routed"
    finally:
        scene.close()


def test_known_answers(routed):
    ramp = routed["ramp"]["got"]
    assert (ramp["direction"][:, :-1] == 0).all() and (ramp["direction"][:, -1] == ref.SINK).all(), "every sample drains east"
    assert (ramp["accumulation"][:, -1] == 17).all() and ramp["sinks"] == 9 and ramp["longest"] == 16 and ramp["rounds"] == 5
    assert np.array_equal(ramp["accumulation"][4], np.arange(1, 18))
    bowl = routed["bowl"]["got"]
    assert bowl["sinks"] == 1 and bowl["accumulation"][4, 4] == 81 and (bowl["basin"] == 4 * 9 + 4).all()
    for name in ("cone 63x65", "cone 33x33"):
        d = routed[name]["got"]["direction"]
        j, i = np.nonzero(d == ref.SINK)
        assert len(j) > 0 and (((j == 0) | (j == d.shape[0] - 1)) | ((i == 0) | (i == d.shape[1] - 1))).all(), "every sink on the border"
    flat = routed["flat"]["got"]
    assert (flat["direction"] == ref.SINK).all() and (flat["accumulation"] == 1).all() and (flat["sinks"], flat["rounds"], flat["longest"]) == (90, 0, 0)
    assert np.array_equal(flat["basin"].reshape(-1), np.arange(90))
    plateau = routed["plateau"]["got"]
    assert plateau["direction"][2, 2] == 0, "four equal slopes: the lowest code, E, wins"
    assert plateau["accumulation"][2, 3] == 2 and plateau["sinks"] == 24 and plateau["rounds"] == 1
    s = routed["serpentine"]["got"]
    assert (s["sinks"], int(s["accumulation"].max()), s["longest"], s["rounds"]) == (1, 1089, 544, 10)
    assert (s["basin"] == 32 * 33 + 32).all() and s["accumulation"][32, 32] == 1089, "one sink: the channel's end (the 17th row runs east)"


@pytest.mark.parametrize("name", ["5x3 x1.0", "33x33 x2.5", "65x63 x2.5", "ramp", "serpentine", "flat"])
def test_stream_records_counts_and_order(harness, routed, name):
    r = routed[name]
    scene = _scene(harness, name)
    try:
        top = int(r["want"]["accumulation"].max())
        for threshold in sorted({1, 2, max(2, top // 8), top, top + 1}):
            whole = ref.streams(r["want"], r["origin"], r["spacing"], threshold)
            for rname, region in cases.regions(r["dem"].shape).items():
                want = ref.streams(r["want"], r["origin"], r["spacing"], threshold, region)
                got = scene.streams(threshold, region)
                assert got["total"] == len(want["segments"]), (threshold, rname)
                assert got["segments"].tobytes() == want["segments"].tobytes(), "coordinates are plane_at's bits, in row-major order"
                assert np.array_equal(got["accumulation"], want["accumulation"])
                row0, col0, rows, cols = region
                j, i = whole["sample"] // r["dem"].shape[1], whole["sample"] % r["dem"].shape[1]
                inside = (j >= row0) & (j < row0 + rows) & (i >= col0) & (i < col0 + cols)
                assert got["segments"].tobytes() == whole["segments"][inside].tobytes(), "a region filters the whole DEM's records"
            if threshold == top + 1:
                assert len(whole["segments"]) == 0
        n = scene.streams(1)["total"]
        assert n == r["dem"].size - r["want"]["sinks"], "threshold 1: every sample that is no sink"
        if n >= 2:
            all_of_them = scene.streams(1, rgba=(0.1, 0.3, 0.8, 1.0))
            half = scene.streams(1, capacity=n // 2)
            assert half["total"] == n and half["segments"].tobytes() == all_of_them["segments"][:n // 2].tobytes()
            want = np.zeros((n, 20), f32)
            want[:, 0:4], want[:, 4:6] = all_of_them["segments"], all_of_them["segments"][:, 2:4]
            want[:, 6:18] = np.tile(np.array([0.1, 0.3, 0.8, 1.0], f32), 3)
            assert all_of_them["prims"].tobytes() == want.view(np.uint32).tobytes(), "v = (a, b, b), one colour, feature 0, reserved 0"
    finally:
        scene.close()


@pytest.mark.parametrize("name", list(CASES))
def test_the_chosen_slope_against_float64(routed, name):
    """Derived, not measured: (1 - 8 x 2^-24).  An f32 slope is the f64 one times (1 + e), |e| <= 4 x 2^-24 to first order -- the
    drop, the diagonal's sum and sqrt, the quotient --; the f32 winner w and the f64 winner m satisfy s32[w] >= s32[m], hence
    s64[w] >= s64[m] (1 - 4u) / (1 + 4u) >= s64[m] (1 - 8u) with the second-order terms inside the last unit's slack (8u exactly
    would need all eight roundings at their bound in the bad direction; (1 - 4u) / (1 + 4u) = 1 - 8u + 32u^2 - ...)."""
    r = routed[name]
    s64 = ref.slopes(r["heights"], r["spacing"], np.float64)
    s64 = np.where(np.isnan(s64), -np.inf, s64)
    code = r["got"]["direction"]
    best = s64.max(0)
    sink = code == ref.SINK
    assert np.array_equal(sink, ~(best > 0.0)), "a positive f64 slope is a positive f32 slope: the sinks coincide"
    chosen = np.take_along_axis(s64, np.minimum(code, 7)[None].astype(np.int64), 0)[0]
    assert (chosen[~sink] >= (1.0 - 8.0 * ULP) * best[~sink]).all()
    choice64 = np.where(sink, ref.SINK, s64.argmax(0))  # (argmax: the lowest index of equals)
    different = int((choice64 != code).sum())
    print(f"{name}: {different} samples where the float32 and the float64 choice differ")
    if name in PROXIES:
        assert different == 0


# ---- the sanitizer run: a stand-alone program, never code loaded into this process ---------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(cases.HARNESS, "drainage_host")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "disagreements: 0" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- the interface -------------------------------------------------------------------------------------------------------------
MEMBERS = {
    "f3d_session_drainage_desc": ["struct_size", "flags", "row0", "col0", "rows", "cols", "direction", "accumulation", "basin", "stats", "ms", "reserved"],
    "f3d_session_streams_desc": ["struct_size", "flags", "row0", "col0", "rows", "cols", "threshold", "reserved", "segments", "accumulation", "capacity",
                                 "total"],
    "f3d_session_paint_streams_desc": ["struct_size", "flags", "row0", "col0", "rows", "cols", "threshold", "reserved", "total", "rgba", "half_width",
                                       "opacity", "aim"],
}
RUST = {"f3d_session_drainage_desc": "F3dSessionDrainageDesc", "f3d_session_streams_desc": "F3dSessionStreamsDesc",
        "f3d_session_paint_streams_desc": "F3dSessionPaintStreamsDesc"}


def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header and _native.ABI_VERSION == 6, "the drainage entry points are additive: no ABI version bump"
    structs = {"f3d_session_drainage_desc": _native.DrainageDesc, "f3d_session_streams_desc": _native.StreamsDesc,
               "f3d_session_paint_streams_desc": _native.PaintStreamsDesc}
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
    assert C.sizeof(_native.DrainageDesc) == 72 == harness.drain_desc_size(0)
    assert C.sizeof(_native.StreamsDesc) == 64 == harness.drain_desc_size(1)
    assert C.sizeof(_native.PaintStreamsDesc) == 64 + C.sizeof(_native.ReaimDesc) == harness.drain_desc_size(2)
    for desc in structs:
        fn = desc[:-5]
        assert re.search(rf"int {fn}\(f3d_session \*session, const {desc} \*desc, char \*err, size_t errlen\);", header)
        entry = [e for e in _native.ABI if e[0] == fn]
        assert len(entry) == 1 and entry[0][1] is C.c_int
    for define, value in (("F3D_DRAINAGE_DEVICE_POINTERS 4u", _native.DRAINAGE_DEVICE_POINTERS), ("F3D_STREAMS_DEVICE_POINTERS 4u", _native.STREAMS_DEVICE_POINTERS)):
        assert f"#define {define}" in header and value == 4 == _native.RASTER_DEVICE_POINTERS
    assert "#define F3D_DRAINAGE_SINK 8u" in header and _native.DRAINAGE_SINK == 8 == ref.SINK
    assert "csrc/f3d_drainage.h" in header, "the ABI header refers to the contract"
    assert "f3d_drainage.hip" in _native.HIP_SOURCES


def test_integration_guide_has_the_structs_and_the_externs():
    text = (ROOT / "INTEGRATION.md").read_text()
    for cname, rust in RUST.items():
        body = re.search(rf"pub struct {rust} \{{(.*?)\n\}}", text, re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == MEMBERS[cname]
        types = {k: v.strip() for k, v in re.findall(r"pub (\w+): ([^,]+),", body)}
        assert all(types[n] == "u32" for n in MEMBERS[cname][:6]) and types["reserved"] == "u32"
        fn = cname[:-5]
        assert re.search(rf"pub fn {fn}\(session: \*mut F3dSession, desc: \*const {rust}, err: \*mut c_char, errlen: usize\) -> c_int;", text)
    assert "pub direction: *mut u8" in text and "pub stats: *mut u32" in text and "pub ms: *mut f64" in text and "pub threshold: u32" in text


def test_the_entry_points_answer_status_4_without_a_device():
    """In a process without a HIP device the three entry points answer F3D_STATUS_DEVICE before any other check -- whatever
    session and descriptor they are handed -- and write nothing.  (With a device the probe passes and the null session is the
    first refusal, status 1; the refusals on a live session are tests/test_gpu_drainage.py's.)"""
    from forge3d_amd import _native

    L = _native.lib()
    have_device = _native.device_count() > 0
    total = C.c_uint64(7)
    stats = (C.c_uint32 * 3)(7, 7, 7)
    d = _native.DrainageDesc()
    d.struct_size, d.stats = C.sizeof(d), C.addressof(stats)
    q = _native.StreamsDesc()
    q.struct_size, q.threshold, q.total = C.sizeof(q), 1, C.addressof(total)
    p = _native.PaintStreamsDesc()
    p.struct_size, p.threshold, p.total = C.sizeof(p), 1, C.addressof(total)
    for call, own in ((L.f3d_session_drainage, d), (L.f3d_session_streams, q), (L.f3d_session_paint_streams, p)):
        for desc in (own, None):  # (its descriptor, or none: the probe comes first)
            err = C.create_string_buffer(256)
            rc = call(None, None if desc is None else C.byref(desc), err, len(err))
            if have_device:
                assert rc == _native.STATUS_VALUE and err.value == b"null session handle"
            else:
                assert rc == _native.STATUS_DEVICE == 4 and err.value == b"no HIP device available: libf3dhip has no CPU fallback"
    assert total.value == 7 and list(stats) == [7, 7, 7]


def _bare_session(dem_shape=(9, 9)):
    from forge3d_amd.session import TerrainSession

    s = TerrainSession.__new__(TerrainSession)
    s.dem_shape = dem_shape
    s._handle = None
    s._device = 0
    return s


def test_wrapper_methods_and_argument_checks(monkeypatch):
    import inspect

    from forge3d_amd.session import TerrainSession
    from forge3d_amd.viewer import ViewerError, ViewerHandle

    p = inspect.signature(TerrainSession.drainage).parameters
    assert list(p) == ["self", "region", "direction", "accumulation", "basin", "out", "wait"] and p["region"].default is None
    assert (p["direction"].default, p["accumulation"].default, p["basin"].default, p["out"].default, p["wait"].default) == (True, True, False, None, True)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("direction", "accumulation", "basin", "out", "wait"))
    for thin in ("flow_directions", "flow_accumulation", "basins"):
        assert list(inspect.signature(getattr(TerrainSession, thin)).parameters) == ["self", "region"]
    q = inspect.signature(TerrainSession.streams).parameters
    assert list(q) == ["self", "threshold", "region", "out"] and all(q[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("region", "out"))
    q = inspect.signature(TerrainSession.paint_streams).parameters
    assert list(q)[:2] == ["self", "threshold"] and q["width"].default == 1.0 and q["opacity"].default == 1.0 and len(q["rgba"].default) == 4
    assert q["rearmable"].kind is inspect.Parameter.VAR_KEYWORD and q["camera"].default is None and q["region"].default is None
    v = inspect.signature(ViewerHandle.enable_streams).parameters
    assert list(v)[:2] == ["self", "threshold"] and (v["width"].default, v["trunk_threshold"].default, v["trunk_width"].default) == (1.5, 0, 3.0)
    assert TerrainSession.DRAINAGE_SINK == 8 and TerrainSession.DRAINAGE_STEPS == ref.STEPS
    _no_device(monkeypatch)
    s = _bare_session()
    with pytest.raises(ValueError, match="drainage\\(\\) always waits"):
        s.drainage(wait=False)
    with pytest.raises(ValueError, match="must not be negative"):
        s.drainage((0, -1, 2, 2))
    with pytest.raises(ValueError, match="out must be None, 'device' or a dict"):
        s.drainage(out="host")
    for call in (s.streams, s.paint_streams):
        for bad in (0, -3, 1.5, 1 << 32):
            with pytest.raises(ValueError, match="threshold is an accumulation"):
                call(bad)
        with pytest.raises(ValueError, match="must not be negative"):
            call(5, region=(0, -1, 2, 2))
    with pytest.raises(ValueError, match="segments must be a contiguous float32 tensor"):
        s.streams(5, out=(np.zeros((4, 4), f32), None))
    with pytest.raises(TypeError, match="unexpected keyword argument 'spp'"):
        s.paint_streams(5, spp=2)
    with pytest.raises(ValueError, match="one colour of 3 or 4 numbers"):
        s.paint_streams(5, rgba=(0.0, 1.0))
    with pytest.raises(ValueError, match="width must be finite and >= 0"):
        s.paint_streams(5, width=-1.0)
    with pytest.raises(ValueError, match=re.escape("opacity must lie in [0, 1]")):
        s.paint_streams(5, opacity=1.5)
    handle = ViewerHandle.__new__(ViewerHandle)
    handle._revision = 0
    for bad in (dict(threshold=0), dict(threshold=2.5), dict(threshold=5, trunk_threshold=-1), dict(threshold=5, width=-1.0),
                dict(threshold=5, rgba=(0.0, 2.0, 0.0))):
        with pytest.raises(ViewerError):
            handle.enable_streams(**bad)
    handle.enable_streams(50, trunk_threshold=500)
    assert handle._streams["threshold"] == 50 and handle._streams["trunk_threshold"] == 500 and handle._revision == 1
    handle.disable_streams()
    assert handle._streams is None and handle._revision == 2


def planes_refusals(call, names, dtypes, shape=(9, 9)):
    """``call(out)``: drainage() or fill() on a bare session of ``shape``.  The planes by name: every text in full."""
    from test_session_contour_host import device_tensor, refused

    under = "out must be None, 'device' or a dict of tensors under " + ", ".join(repr(n) for n in names)
    refused(under, call, "host")
    refused(under, call, "")
    refused(under, call, {"height": None})
    refused(under, call, {names[0]: device_tensor(shape, dtypes[0]), "height": None})
    for name, dtype in zip(names, dtypes):
        text = f"out[{name!r}] must be a contiguous torch.{dtype} tensor ({shape[0]}, {shape[1]}) on the session's device"
        other = "float64" if dtype != "float64" else "int32"
        for plane in (np.zeros(shape), device_tensor((shape[0], shape[1] + 1), dtype), device_tensor((shape[0] * shape[1],), dtype),
                      device_tensor(shape, other), device_tensor(shape, dtype, contiguous=False)):
            refused(text, call, {name: plane})


def test_shared_refusals_of_the_planes_the_record_outputs_and_the_stroke_in_the_drainage_words(monkeypatch):
    from test_session_contour_host import UntouchedLibrary, record_outputs_refusals, stroke_refusals

    _no_device(monkeypatch)
    s = _bare_session()
    s._lib = UntouchedLibrary()
    assert [n for n, _, _ in s._DRAINAGE_PLANES] == ["direction", "accumulation", "basin"]
    nothing = dict(direction=False, accumulation=False)  # (a plane that is wanted and not given is allocated on the way: on a device)
    for call in (lambda out: s.drainage(out=out, **nothing), lambda out: s.filled.drainage(out=out, **nothing)):
        planes_refusals(call, ("direction", "accumulation", "basin"), ("uint8", "int32", "int32"))
    for streams in (s.streams, s.filled.streams):
        record_outputs_refusals(lambda out: streams(5, out=out), "accumulation")
    for paint in (s.paint_streams, s.filled.paint_streams):
        stroke_refusals(lambda **stroke: paint(5, **stroke))
