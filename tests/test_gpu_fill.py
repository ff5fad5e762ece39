"""Drainage through depressions on a live session (f3d_session_fill, F3D_DRAINAGE_FILL), on the device.

* fill(), filled.drainage() and filled.streams() return the bits of the host build of the lane and tile bodies (tests/fill_host,
  the device's tile edge, tiles in index order) -- every plane on its own, with the counts -- in the host form and in the device
  form, for every region of fill_cases' DEMs: the 63x65 and 65x130 reliefs, the nested depression, the flat, and the walled
  serpentines of 35x35 and (2 TILE + 3)^2, the largest input.  The fill and flat round counts come back and are >= 1 where there
  is anything to relax; they are not compared with the host's (a device schedule may need fewer);
* two calls in a row return the same bits; without the fill the calls return what they returned before (tests/drainage_host);
* on 63x65 plain drainage() has interior sinks; the filled routing has none, its basins are all outlets and its sinks'
  accumulations sum to w * h;
* after a reterrain that opens a dam, fill() equals a fresh session's;
* paint_streams(t, fill=True) leaves drape_image() bit-identical to paint(filled.streams(t)["segments"]);
* the fill entry's refusals in the header's order, 0x40 unknown on all four entries; each leaves fingerprint() and
  drape_image() as they were.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import drainage_cases as cases
import fill_cases
from test_gpu_drainage import _equal, _equal_streams, _paint_segments, _session
from test_session_drape_host import drape_dem, drape_kw, random_image

pytestmark = pytest.mark.gpu

f32 = np.float32
FILL_PLANES = ("filled", "depth", "flat_distance")


@pytest.fixture(scope="module")
def harness():
    return fill_cases.build_harness()


@pytest.fixture(scope="module")
def gpu_cases(harness):
    tile = int(harness.fill_tile_edge())
    named, extra = cases.named_cases(), fill_cases.extra_cases(tile)
    big = f"walled serpentine {2 * tile + 3}"
    assert extra[big][0].shape == (2 * tile + 3, 2 * tile + 3)
    return {"63x65": named["65x63 x2.5"], "relief 65x130": extra["relief 65x130"], "nested": extra["nested"], "flat": named["flat"],
            "walled serpentine 35x35": extra["walled serpentine 35x35"], "walled serpentine, 3 x 3 tiles": extra[big]}


NAMES = ["63x65", "relief 65x130", "nested", "flat", "walled serpentine 35x35", "walled serpentine, 3 x 3 tiles"]


def _host(harness, case):
    dem, spacing, e = case
    kw = cases.shape_kw(dem, spacing, e)
    return fill_cases.HostFill(harness, dem, kw), dem, kw


def _cut(whole, region, planes):
    row0, col0, rows, cols = region
    return {k: (v[row0:row0 + rows, col0:col0 + cols] if k in planes else v) for k, v in whole.items()}


def _equal_fill(got, want, what):
    for plane in FILL_PLANES:
        a = got[plane].cpu().numpy() if hasattr(got[plane], "cpu") else got[plane]
        assert a.shape == want[plane].shape and a.view(np.uint32).tobytes() == np.ascontiguousarray(want[plane]).view(np.uint32).tobytes(), (what, plane)
    for word in ("filled_samples", "largest_flat_distance"):
        assert got[word] == want[word], (what, word, got[word], want[word])
    assert got["fill_rounds"] >= 1 and got["flat_rounds"] >= min(1, want["flat_rounds"]), (what, got["fill_rounds"], got["flat_rounds"])


def _numpy(got, planes):
    return {k: (v.cpu().numpy().view(np.uint8 if k == "direction" else np.uint32) if k in planes else v) for k, v in got.items()}


@pytest.mark.parametrize("name", NAMES)
def test_the_device_returns_the_bits_of_the_host_body(harness, gpu_cases, name):
    host, dem, kw = _host(harness, gpu_cases[name])
    try:
        fill, routed = host.fill(), host.drainage()
        top = int(routed["accumulation"].max())
        with _session(dem, kw) as s:
            for rname, region in cases.regions(dem.shape).items():
                what = f"{name}, {rname}"
                want = _cut(fill, region, FILL_PLANES)
                _equal_fill(s.fill(region, depth=True, flat_distance=True), want, what)
                _equal_fill(s.fill(region, depth=True, flat_distance=True, out="device"), want, what + ", device form")
                want = _cut(routed, region, cases_planes())
                _equal(s.filled.drainage(region, basin=True), want, what)
                _equal(_numpy(s.filled.drainage(region, basin=True, out="device"), cases_planes()), want, what + ", device form")
                for threshold in sorted({1, max(2, top // 8), top + 1}):
                    _equal_streams(s.filled.streams(threshold, region=region), host.streams(threshold, region), f"{what}, threshold {threshold}")
            assert np.array_equal(s.filled_heights(), fill["filled"]) and np.array_equal(s.lake_depth(), fill["depth"])
            assert np.array_equal(s.filled.flow_directions(), routed["direction"]) and np.array_equal(s.filled.flow_accumulation(), routed["accumulation"])
            assert np.array_equal(s.filled.basins(), routed["basin"])
            only = s.fill(filled=False)
            assert set(only) == {"filled_samples", "fill_rounds", "flat_rounds", "largest_flat_distance"} and only["filled_samples"] == fill["filled_samples"]
    finally:
        host.close()


def cases_planes():
    return ("direction", "accumulation", "basin")


def test_the_device_form_of_the_streams_and_guard_rows(harness, gpu_cases):
    import torch

    host, dem, kw = _host(harness, gpu_cases["relief 65x130"])
    try:
        want = host.streams(4)
        n = want["total"]
        region = (5, 3, 13, 15)
        part = _cut(host.fill(), region, FILL_PLANES)
        with _session(dem, kw) as s:
            device = torch.device("cuda", torch.cuda.current_device())
            d_seg = torch.full((n + 8, 4), 77.0, dtype=torch.float32, device=device)
            d_acc = torch.full((n + 8,), 77, dtype=torch.int32, device=device)
            got = s.filled.streams(4, out=(d_seg[:n + 3], d_acc[:n + 3]))
            assert got["total"] == n and got["segments"].cpu().numpy().tobytes() == want["segments"].tobytes()
            assert np.array_equal(got["accumulation"].cpu().numpy().view(np.uint32), want["accumulation"])
            assert bool((d_seg[n:] == 77.0).all()) and bool((d_acc[n:] == 77).all())
            guard = torch.full((15, 15), 77.0, dtype=torch.float32, device=device)
            mine = s.fill(region, filled=False, out={"depth": guard[1:14]})
            assert set(mine) == {"depth", "filled_samples", "fill_rounds", "flat_rounds", "largest_flat_distance"}
            assert np.array_equal(guard[1:14].cpu().numpy(), part["depth"]) and bool((guard[0] == 77.0).all()) and bool((guard[14] == 77.0).all())
    finally:
        host.close()


def test_two_calls_in_a_row_and_the_calls_without_the_fill(harness, gpu_cases):
    """The same bits twice; and behind filled calls, on the same session, the plain calls return tests/drainage_host's bits --
    what they returned before the fill existed."""
    host, dem, kw = _host(harness, gpu_cases["63x65"])
    plain = cases.HostDrainage(cases.build_harness(), dem, kw)
    try:
        with _session(dem, kw) as s:
            a, b = s.fill(depth=True, flat_distance=True), s.fill(depth=True, flat_distance=True)
            for plane in FILL_PLANES:
                assert a[plane].tobytes() == b[plane].tobytes(), plane
            assert (a["filled_samples"], a["largest_flat_distance"]) == (b["filled_samples"], b["largest_flat_distance"])
            _equal(s.filled.drainage(basin=True), s.filled.drainage(basin=True), "twice")
            _equal_streams(s.filled.streams(3), s.filled.streams(3), "twice")
            _equal(s.drainage(basin=True), plain.run(), "fill off")
            _equal(s.drainage(basin=True), host.drainage(edge=0), "fill off, this harness")
            _equal_streams(s.streams(3), plain.streams(3), "fill off")
            _equal(s.filled.drainage(basin=True), host.drainage(), "and on again")
    finally:
        host.close()
        plain.close()


def test_the_filled_routing_has_no_interior_sinks(gpu_cases):
    dem, spacing, e = gpu_cases["63x65"]
    rows, cols = dem.shape
    j, i = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    border = (j == 0) | (j == rows - 1) | (i == 0) | (i == cols - 1)
    with _session(dem, cases.shape_kw(dem, spacing, e)) as s:
        plain = s.drainage(basin=True)
        assert int(((plain["direction"] == s.DRAINAGE_SINK) & ~border).sum()) > 0, "the DEM has pits: rivers end inside it"
        got = s.filled.drainage(basin=True)
        sink = got["direction"] == s.DRAINAGE_SINK
        assert not (sink & ~border).any() and got["sinks"] == int(sink.sum()) > 0
        assert border.reshape(-1)[got["basin"].reshape(-1)].all(), "every basin is an outlet"
        assert int(got["accumulation"][sink].astype(np.int64).sum()) == rows * cols
        assert int(got["accumulation"].max()) > int(plain["accumulation"].max()), "the rivers no longer end in the pits"


def test_after_a_reterrain_that_opens_a_dam_fill_equals_a_fresh_sessions(harness):
    dem = np.full((20, 24), 50.0, f32)
    dem[3:17, 3:21] = 10.0      # a basin behind a dam all round
    dem[:, 0] = dem[:, -1] = 40.0
    opened = dem.copy()
    opened[8:11, 20:24] = np.array([12.0, 11.5, 11.0, 5.0], f32)  # the block that breaches the east dam down to the border
    kw = cases.shape_kw(dem, (10.0, 7.0), 1.0)
    with _session(dem, kw) as s:
        before = s.fill(depth=True)
        assert before["filled_samples"] == 14 * 18 and before["depth"].max() == 40.0
        s.reterrain(opened[8:11, 20:24], at=(8, 20))
        got = s.fill(depth=True, flat_distance=True)
        host = fill_cases.HostFill(harness, opened, kw)
        try:
            _equal_fill(got, host.fill(), "after reterrain")
            _equal(s.filled.drainage(basin=True), host.drainage(), "after reterrain")
        finally:
            host.close()
        with _session(opened, kw) as fresh:
            want = fresh.fill(depth=True, flat_distance=True)
            for plane in FILL_PLANES:
                assert got[plane].tobytes() == want[plane].tobytes(), plane
        assert got["depth"].max() < 40.0, "the lake fell to the breach"


def test_paint_streams_with_fill_leaves_the_bits_of_the_host_route():
    dem = fill_cases.relief((33, 40), 5)
    kw = drape_kw(dem)
    style = dict(rgba=(0.1, 0.3, 0.8, 0.9), width=1.7 * kw["spacing"][0] * (dem.shape[1] - 1) / 130, opacity=0.9)
    with _session(dem, kw) as a, _session(dem, kw) as b:
        for s in (a, b):
            s.drape(random_image((70, 130), 95), filter="nearest")
        before = a.drape_image()
        for region, threshold in ((None, 3), ((3, 2, 9, 11), 1)):
            n = a.paint_streams(threshold, region=region, fill=True, **style)
            got = b.filled.streams(threshold, region=region)
            assert n == got["total"] > 10
            _paint_segments(b, got, style)
            painted = a.drape_image()
            assert painted.tobytes() == b.drape_image().tobytes(), region
        assert (painted != before).any(-1).mean() > 0.02, "the streams are visible"
        assert a.filled.paint_streams(3, **style) == b.paint_streams(3, fill=True, **style)
        assert a.drape_image().tobytes() == b.drape_image().tobytes()


def _raw_fill(s, /, **members):
    from forge3d_amd import _native

    stats = (C.c_uint32 * 4)(99, 99, 99, 99)
    q = _native.FillDesc()
    q.struct_size = C.sizeof(q)
    q.row0, q.col0, q.rows, q.cols = 0, 0, s.dem_shape[0], s.dem_shape[1]
    q.stats = C.addressof(stats)
    for k, v in members.items():
        setattr(q, k, v)
    err = C.create_string_buffer(1024)
    rc = s._lib.f3d_session_fill(s._handle, C.byref(q), err, len(err))
    return rc, err.value.decode(), list(stats)


def test_every_refusal_in_its_order_leaves_the_session_and_the_canvas_as_they_were():
    from test_gpu_drainage import _raw

    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    dem_h, dem_w = dem.shape
    refusals = [
        ("the struct size", dict(struct_size=8), ".struct_size is 8"),
        ("unknown flags", dict(flags=0x40), "unknown fill flags 0x40"),
        ("the drainage's FILL flag", dict(flags=8), "unknown fill flags 0x8"),
        ("reserved", dict(reserved=3), "reserved member must be 0, got 3"),
        ("an empty region", dict(rows=0), "empty fill region: 0 rows"),
        ("a region outside the DEM", dict(row0=dem_h), f"lies outside the {dem_h}x{dem_w} DEM"),
        ("a misaligned device plane", dict(flags=4, depth=6), "4-byte aligned"),
    ]
    with _session(dem, kw) as s:
        s.drape(random_image((24, 40), 96))
        s.enqueue_frames(0, 1)
        state = lambda: (s.fingerprint(), s.drape_info(), s.drape_image().tobytes())  # noqa: E731
        before = state()
        for what, members, text in refusals:
            rc, message, stats = _raw_fill(s, **members)
            assert rc == 1 and text in message, (what, rc, message)
            assert stats == [99] * 4 and state() == before, what
        # the order: of two causes the earlier one's message wins
        for members, text in ((dict(struct_size=8, flags=0x40), ".struct_size is 8"), (dict(flags=0x40, reserved=3), "unknown fill flags"),
                              (dict(reserved=3, rows=0), "reserved member"), (dict(rows=0, row0=dem_h), "empty fill region"),
                              (dict(flags=4, row0=dem_h, filled=6), "lies outside")):
            rc, message, _ = _raw_fill(s, **members)
            assert rc == 1 and text in message, (members, message)
        for which in ("drainage", "streams", "paint"):
            rc, message, total, stats = _raw(s, which, flags=0x40)
            assert rc == 1 and "unknown drainage flags 0x40" in message and total == 99 and stats == [99, 99, 99], which
            rc, message, _, _ = _raw(s, which, flags=0x48)
            assert rc == 1 and "unknown drainage flags 0x48" in message, "FILL beside an unknown bit is still refused"
        assert state() == before
        rc, _, stats = _raw_fill(s, stats=None)
        assert rc == 0, "every output of the fill entry may be null"
        rc, message, stats = _raw_fill(s)
        assert rc == 0 and stats[1] >= 1 and state() == before, "a query: the render and the canvas go on as they were"
        for which in ("drainage", "streams"):
            assert _raw(s, which, flags=8)[0] == 0, which
        with pytest.raises(ValueError, match="lies outside"):
            s.fill((0, 0, dem_h + 1, dem_w))
        assert state() == before
        assert _raw(s, "paint", flags=8)[0] == 0 and state()[2] != before[2], "what is accepted after all that paints"
