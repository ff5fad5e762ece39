"""Drainage on a live session (f3d_session_drainage, f3d_session_streams, f3d_session_paint_streams), on the device.

* drainage() returns the bits of the host build of the lane bodies (tests/drainage_host: the direction pass by tiles, the rounds
  as Jacobi sweeps) -- every plane compared on its own, with sinks, rounds and longest -- for drainage_cases' DEMs and regions;
  streams() returns that build's records, in order and in number;
* a capacity below the total returns the prefix and leaves guard words behind it untouched; the device forms equal the host forms;
* state that outlives a call: a large call, then a small one; after reterrain (whole, with at=, with a new exaggeration) the
  result is a fresh session's on the new DEM; a strip session returns the whole DEM's drainage;
* paint_streams() leaves drape_image() bit-identical to a twin session that ran paint(streams()["segments"]) with the same
  style -- on the square canvas and on the flipped anisotropic canvas of the paint tests -- and the two render the same bits in
  every AOV; a threshold above w * h leaves the drape's bits;
* every refusal, in its order, with its message, leaves fingerprint() and drape_image() as they were;
* ViewerHandle.enable_streams renders what the equivalent drape and paint_streams calls render.
Every render is 64x48 with two frames; 65x63 and the 33x33 serpentine are the largest inputs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import drainage_cases as cases
import scenes
from test_session_drape_host import CAM, drape_dem, drape_kw, random_image
from test_session_paint_host import ANISO, SQUARE, flipped

pytestmark = pytest.mark.gpu

W, H = cases.SIZE
AOVS = ("rgba", "albedo", "normal", "depth")
PLANES = ("direction", "accumulation", "basin")
f32 = np.float32
CASES = cases.named_cases()


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or CAM), **opts, **kw)


def _frames(s, n=2):
    s.enqueue_frames(0, n)
    return s.resolve(n)


def _same(got, want, what):
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key}"


def _equal(got, want, what):
    for plane in PLANES:
        assert got[plane].dtype == want[plane].dtype and got[plane].shape == want[plane].shape, (what, plane)
        assert np.array_equal(got[plane], want[plane]), (what, plane)
    for word in ("sinks", "rounds", "longest"):
        assert got[word] == want[word], (what, word, got[word], want[word])


def _equal_streams(got, want, what):
    assert got["total"] == want["total"], what
    assert got["segments"].tobytes() == want["segments"].tobytes(), what
    assert np.array_equal(got["accumulation"], want["accumulation"]), what


@pytest.fixture(scope="module")
def harness():
    return cases.build_harness()


@pytest.mark.parametrize("name", list(CASES))
def test_the_device_returns_the_bits_of_the_host_body(harness, name):
    dem, spacing, e = CASES[name]
    kw = cases.shape_kw(dem, spacing, e)
    host = cases.HostDrainage(harness, dem, kw)
    try:
        with _session(dem, kw) as s:
            whole = None
            for rname, region in cases.regions(dem.shape).items():
                want = host.run(region)
                _equal(s.drainage(region, basin=True), want, f"{name}, {rname}")
                whole = want if rname == "whole" else whole
                top = int(whole["accumulation"].max())
                for threshold in sorted({1, max(2, top // 8), top + 1}):
                    _equal_streams(s.streams(threshold, region=region), host.streams(threshold, region), f"{name}, {rname}, threshold {threshold}")
            assert np.array_equal(s.flow_directions(), whole["direction"]) and np.array_equal(s.flow_accumulation(), whole["accumulation"])
            assert np.array_equal(s.basins(), whole["basin"])
            only = s.drainage(direction=False, accumulation=False)
            assert set(only) == {"sinks", "rounds", "longest"} and only["rounds"] == whole["rounds"]
    finally:
        host.close()


def test_capacity_guard_words_and_the_device_forms(harness):
    import torch

    from forge3d_amd import _native

    dem, spacing, e = CASES["65x63 x2.5"]
    kw = cases.shape_kw(dem, spacing, e)
    host = cases.HostDrainage(harness, dem, kw)
    try:
        want = host.streams(2)
        n, cap = want["total"], want["total"] // 3
        assert cap > 64
        routed = host.run()
        with _session(dem, kw) as s:
            seg, acc = np.full((cap + 8, 4), 77.0, f32), np.full(cap + 8, 77, np.uint32)
            total = C.c_uint64(0)
            q = _native.StreamsDesc()
            q.struct_size = C.sizeof(q)
            q.row0, q.col0, q.rows, q.cols = 0, 0, dem.shape[0], dem.shape[1]
            q.threshold = 2
            q.segments, q.accumulation, q.capacity, q.total = seg.ctypes.data, acc.ctypes.data, cap, C.addressof(total)
            assert s._lib.f3d_session_streams(s._handle, C.byref(q), s._err, len(s._err)) == 0, s._err.value
            assert total.value == n and seg[:cap].tobytes() == want["segments"][:cap].tobytes() and np.array_equal(acc[:cap], want["accumulation"][:cap])
            assert (seg[cap:] == 77.0).all() and (acc[cap:] == 77).all(), "guard words behind the capacity are untouched"
            q.segments, q.accumulation, q.capacity = None, None, 0
            assert s._lib.f3d_session_streams(s._handle, C.byref(q), s._err, len(s._err)) == 0 and total.value == n, "null outputs size the next call"
            device = torch.device("cuda", torch.cuda.current_device())
            for room in (n + 5, cap):
                d_seg = torch.full((room + 8, 4), 77.0, dtype=torch.float32, device=device)
                d_acc = torch.full((room + 8,), 77, dtype=torch.int32, device=device)
                got = s.streams(2, out=(d_seg[:room], d_acc[:room]))
                k = min(n, room)
                assert got["total"] == n and tuple(got["segments"].shape) == (k, 4)
                assert got["segments"].cpu().numpy().tobytes() == want["segments"][:k].tobytes()
                assert np.array_equal(got["accumulation"].cpu().numpy().view(np.uint32), want["accumulation"][:k])
                assert bool((d_seg[k:] == 77.0).all()) and bool((d_acc[k:] == 77).all())
            only = s.streams(2, out=(torch.empty((n, 4), dtype=torch.float32, device=device), None))
            assert only["accumulation"] is None and only["segments"].cpu().numpy().tobytes() == want["segments"].tobytes()
            monkey_room = s.STREAMS_FIRST_CAPACITY
            try:
                s.STREAMS_FIRST_CAPACITY = 16  # (the host form's second call, for a network larger than its first room)
                _equal_streams(s.streams(2), want, "a second call")
            finally:
                s.STREAMS_FIRST_CAPACITY = monkey_room
            # drainage(): the device form into tensors of the caller's and of its own, a region with guard rows around it
            region = (5, 3, 13, 15)
            part = host.run(region)
            got = s.drainage(region, basin=True, out="device")
            for plane in PLANES:
                assert np.array_equal(got[plane].cpu().numpy().view(part[plane].dtype), part[plane]), plane
            guard = torch.full((15, 15), 77, dtype=torch.int32, device=device)
            mine = s.drainage(region, direction=False, out={"accumulation": guard[1:14]})
            assert set(mine) == {"accumulation", "sinks", "rounds", "longest"} and mine["accumulation"].data_ptr() == guard[1:14].data_ptr()
            assert np.array_equal(guard[1:14].cpu().numpy().view(np.uint32), part["accumulation"]) and bool((guard[0] == 77).all()) and bool((guard[14] == 77).all())
            assert (mine["sinks"], mine["rounds"], mine["longest"]) == (routed["sinks"], routed["rounds"], routed["longest"])
    finally:
        host.close()


def test_state_that_outlives_a_call(harness):
    """A large call, then a small one; reterrain whole, with at=, with a new exaggeration: always a fresh session's result."""
    dem, spacing, e = CASES["65x63 x2.5"]
    kw = cases.shape_kw(dem, spacing, e)

    def fresh(d, k, region=None, threshold=3):
        host = cases.HostDrainage(harness, d, k)
        try:
            return host.run(region), host.streams(threshold, region)
        finally:
            host.close()

    def check(s, d, k, what, region=None):
        want, want_streams = fresh(d, k, region)
        _equal(s.drainage(region, basin=True), want, what)
        _equal_streams(s.streams(3, region=region), want_streams, what)

    with _session(dem, kw) as s:
        check(s, dem, kw, "a large call")
        check(s, dem, kw, "then a small one", (5, 3, 13, 15))
        dem2 = (dem * f32(0.7) + f32(0.2) * np.roll(dem, 5, 1)).astype(f32)
        s.reterrain(dem2)
        check(s, dem2, kw, "after reterrain")
        patch = (dem2[10:31, 20:45] + f32(0.3)).astype(f32)
        dem3 = dem2.copy()
        dem3[10:31, 20:45] = patch
        s.reterrain(patch, at=(10, 20))
        check(s, dem3, kw, "after reterrain at=")
        s.reterrain(dem3, exaggeration=1.0)
        check(s, dem3, dict(kw, exaggeration=1.0), "after reterrain with a new exaggeration")
        snake = cases.serpentine()
        pad = np.full(dem.shape, 1000.0, f32)
        pad[:33, :33] = snake
        s.reterrain(pad)
        check(s, pad, dict(kw, exaggeration=1.0), "ten rounds after six")
        assert s.drainage(direction=False, accumulation=False)["rounds"] == 10


def test_a_strip_session_returns_the_whole_dems_drainage(harness):
    dem, spacing, e = CASES["33x33 x2.5"]
    kw = cases.shape_kw(dem, spacing, e)
    host = cases.HostDrainage(harness, dem, kw)
    try:
        with _session(dem, kw, row_begin=16, row_end=32) as s:
            _equal(s.drainage(basin=True), host.run(), "strip")
            _equal_streams(s.streams(4), host.streams(4), "strip")
    finally:
        host.close()


def _canvas(s, dem_shape, canvas, kind, seed):
    reg = flipped(dem_shape, canvas) if kind == "flipped" else s.drape_registration(canvas[0], canvas[1], kind)
    s.drape(random_image(canvas, seed), registration=tuple(float(v) for v in reg), filter="nearest")


def _paint_segments(s, got, style):
    n = got["total"]
    s.paint(got["segments"].reshape(-1, 2), style["rgba"], primitive="lines", indices=np.arange(2 * n, dtype=np.uint32), width=style["width"],
            opacity=style["opacity"])


@pytest.mark.parametrize("dem_case,canvas,kind", [(SQUARE, (70, 130), "area"), (ANISO, (257, 64), "flipped")], ids=["square-70x130", "aniso-257x64-flipped"])
def test_paint_streams_leaves_the_bits_of_the_host_route(dem_case, canvas, kind):
    dem_shape, spacing = dem_case
    dem = drape_dem(dem_shape)
    kw = dict(drape_kw(dem), spacing=spacing)
    style = dict(rgba=(0.1, 0.3, 0.8, 0.9), width=1.7 * spacing[0] * (dem_shape[1] - 1) / canvas[1], opacity=0.9)
    with _session(dem, kw) as a, _session(dem, kw) as b:
        _canvas(a, dem_shape, canvas, kind, 91)
        _canvas(b, dem_shape, canvas, kind, 91)
        before = a.drape_image()
        for region, threshold in ((None, 3), ((3, 2, 9, 11), 1)):
            n = a.paint_streams(threshold, region=region, **style)
            got = b.streams(threshold, region=region)
            assert n == got["total"] > 10
            _paint_segments(b, got, style)
            painted = a.drape_image()
            assert painted.tobytes() == b.drape_image().tobytes(), region
        assert (painted != before).any(-1).mean() > 0.02, "the streams are visible"
        assert a.paint_streams(dem.size + 1, **style) == 0 and a.drape_image().tobytes() == painted.tobytes(), "a threshold above w * h: the drape keeps its bits"
        assert a.paint_stats()["primitives"] == n


def test_the_two_routes_render_the_same_bits():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    image = random_image((48, 80), 92)
    style = dict(rgba=(0.1, 0.3, 0.8, 1.0), width=1.5, opacity=1.0)
    with _session(dem, kw) as a, _session(dem, kw) as b, _session(dem, kw) as plain:
        for s in (a, b, plain):
            s.drape(image)
        a.enqueue_frames(0, 1)  # (frames in flight over the old canvas: the paint is ordered behind them and restarts the render)
        n = a.paint_streams(2, **style)
        got = b.streams(2)
        assert n == got["total"] > 50
        _paint_segments(b, got, style)
        assert a.drape_image().tobytes() == b.drape_image().tobytes()
        assert a.fingerprint() == b.fingerprint()
        fa = _frames(a)
        _same(fa, _frames(b), "paint_streams against streams + paint")
        assert not np.array_equal(fa["albedo"], _frames(plain)["albedo"]), "the streams are visible"


def _raw(s, which, /, **members):
    """The entry `which` ("drainage", "streams", "paint") with a descriptor of the caller's: (status, message, total, stats)."""
    from forge3d_amd import _native

    total = C.c_uint64(99)
    stats = (C.c_uint32 * 3)(99, 99, 99)
    q = {"drainage": _native.DrainageDesc, "streams": _native.StreamsDesc, "paint": _native.PaintStreamsDesc}[which]()
    q.struct_size = C.sizeof(q)
    q.row0, q.col0, q.rows, q.cols = 0, 0, s.dem_shape[0], s.dem_shape[1]
    if which == "drainage":
        q.stats = C.addressof(stats)
    else:
        q.threshold, q.total = 2, C.addressof(total)
    if which == "paint":
        q.rgba = (C.c_float * 4)(0.1, 0.3, 0.8, 1.0)
        q.half_width, q.opacity = 1.0, 1.0
        q.aim = s._aim(None, {})
    for k, v in members.items():
        setattr(q, k, v)
    err = C.create_string_buffer(1024)
    entry = {"drainage": s._lib.f3d_session_drainage, "streams": s._lib.f3d_session_streams, "paint": s._lib.f3d_session_paint_streams}[which]
    rc = entry(s._handle, C.byref(q), err, len(err))
    return rc, err.value.decode(), int(total.value), list(stats)


def test_every_refusal_in_its_order_leaves_the_session_and_the_canvas_as_they_were():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    dem_h, dem_w = dem.shape
    nan = float("nan")
    shared = [
        ("the struct size", dict(struct_size=8), ".struct_size is 8"),
        ("unknown flags", dict(flags=64), "unknown drainage flags 0x40"),
        ("reserved", dict(reserved=3), "reserved member must be 0, got 3"),
        ("an empty region", dict(rows=0), "empty drainage region: 0 rows"),
        ("a region outside the DEM", dict(row0=dem_h), f"lies outside the {dem_h}x{dem_w} DEM"),
        ("a region one column too wide", dict(col0=1), f"lies outside the {dem_h}x{dem_w} DEM"),
    ]
    own = {
        "drainage": [("null stats", dict(stats=None), "null stats for a drainage call")],
        "streams": [("threshold 0", dict(threshold=0), "at least 1, got 0"), ("a null total", dict(total=None), "null total for a stream call")],
    }
    own["paint"] = own["streams"]
    with _session(dem, kw) as s:
        fp = s.fingerprint()
        rc, message, _, _ = _raw(s, "paint")
        assert rc == 1 and message == "this session has no drape: streams are painted into one (f3d_session_drape gives the canvas)"
        with pytest.raises(ValueError, match="this session has no drape"):
            s.paint_streams(2)
        assert s.fingerprint() == fp and not s.draped
        assert _raw(s, "streams")[0] == 0 and _raw(s, "drainage")[0] == 0, "the queries need no drape"
        s.drape(random_image((24, 40), 93))
        s.enqueue_frames(0, 1)
        state = lambda: (s.fingerprint(), s.drape_info(), s.drape_image().tobytes())  # noqa: E731
        before = state()
        for which in ("drainage", "streams", "paint"):
            for what, members, text in shared + own[which]:
                rc, message, total, stats = _raw(s, which, **members)
                assert rc == 1 and text in message, (which, what, rc, message)
                assert total == 99 and stats == [99, 99, 99] and state() == before, (which, what)
            # the order: of two causes the earlier one's message wins
            last = dict(stats=None) if which == "drainage" else dict(threshold=0)
            for members, text in ((dict(struct_size=8, flags=64), ".struct_size is 8"), (dict(flags=64, reserved=3), "unknown drainage flags"),
                                  (dict(reserved=3, rows=0), "reserved member"), (dict(rows=0, row0=dem_h), "empty drainage region"),
                                  (dict(row0=dem_h, **last), "lies outside")):
                rc, message, _, _ = _raw(s, which, **members)
                assert rc == 1 and text in message, (which, members, message)
            assert state() == before
        rc, message, _, _ = _raw(s, "streams", threshold=0, total=None)
        assert "at least 1" in message, "the threshold, then the total"
        rc, message, _, _ = _raw(s, "paint", total=None, half_width=-1.0)
        assert "null total" in message, "the shared checks come before the paint's own"
        rc, message, _, _ = _raw(s, "drainage", flags=4, accumulation=6)
        assert rc == 1 and "4-byte aligned" in message
        rc, message, _, _ = _raw(s, "streams", capacity=4)
        assert rc == 1 and "null segments for a stream call with room for 4" in message
        seg = np.zeros((4, 4), f32)
        rc, _, total, _ = _raw(s, "streams", segments=seg.ctypes.data, capacity=0)
        assert rc == 0 and total > 0 and not seg.any(), "a non-null output with capacity 0 is legal"
        rc, message, _, _ = _raw(s, "streams", flags=4, segments=8, capacity=4)
        assert rc == 1 and "16-byte aligned" in message
        painted = [
            ("a negative width", dict(half_width=-1.0), 1, "paint half_width must be finite and >= 0"),
            ("a NaN width", dict(half_width=nan), 1, "paint half_width must be finite and >= 0"),
            ("an opacity above 1", dict(opacity=1.25), 1, "paint opacity must lie in [0, 1]"),
            ("an alpha above 1", dict(rgba=(C.c_float * 4)(0.0, 0.0, 0.0, 1.5)), 3, "paint colours must lie in [0, 1]"),
            ("a NaN colour", dict(rgba=(C.c_float * 4)(nan, 0.0, 0.0, 1.0)), 3, "paint colours must lie in [0, 1]"),
        ]
        for what, members, status, text in painted:
            rc, message, total, _ = _raw(s, "paint", **members)
            assert rc == status and text in message, (what, rc, message)
            assert total == 99 and state() == before, what
        rc, message, _, _ = _raw(s, "paint", half_width=-1.0, opacity=2.0, rgba=(C.c_float * 4)(2.0, 0.0, 0.0, 1.0))
        assert "half_width" in message, "half_width, then opacity, then rgba"
        rc, message, _, _ = _raw(s, "paint", opacity=2.0, rgba=(C.c_float * 4)(2.0, 0.0, 0.0, 1.0))
        assert "opacity" in message
        with pytest.raises(ValueError, match="lies outside"):
            s.paint_streams(2, region=(0, 0, dem_h + 1, dem_w))
        assert state() == before
        assert s.paint_streams(2) > 0 and state()[2] != before[2], "what is accepted after all that paints"
    # the reach: a canvas so fine that the DEM's corner lies more than 2^16 texels from the centre
    with _session(dem, kw) as s:
        s.drape(random_image((8, 8), 94), registration=(4200.0, -0.5, 4200.0, -0.5), filter="nearest")
        before = s.fingerprint(), s.drape_image().tobytes()
        rc, message, total, _ = _raw(s, "paint")
        assert rc == 3 and "the stream region reaches more than 65536 texels of the drape" in message and total == 99
        assert (s.fingerprint(), s.drape_image().tobytes()) == before
        rc, _, _, _ = _raw(s, "paint", row0=14, col0=14, rows=4, cols=4)
        assert rc == 0, "a region near the centre is inside the reach"


def test_enable_streams_renders_what_the_equivalent_calls_render():
    from forge3d_amd.session import TerrainSession
    from forge3d_amd.viewer import ViewerHandle

    dem = drape_dem()
    v = ViewerHandle(W, H, spp=2, max_frames=2, min_frames=2, variance_threshold=1e30)
    spacing = scenes.SPAN / (dem.shape[1] - 1)
    v.load_terrain(dem, spacing)
    v.set_z_scale(scenes.RELIEF)
    v.set_orbit_camera(phi_deg=28.0, theta_deg=49.0, radius=120.0, fov_deg=60.0)
    plain = v.render()
    v.enable_contours(2.0, base=0.5, width=1.5, rgba=(0.2, 0.1, 0.0, 0.8))
    v.enable_streams(3, width=1.5, rgba=(0.1, 0.3, 0.8, 1.0), trunk_threshold=12, trunk_width=3.0)
    got = v.render()
    assert not np.array_equal(got["albedo"], plain["albedo"])

    d, w, h, camera, keywords = v._call()
    with TerrainSession(d, w, h, camera, **keywords) as s:
        rows, cols = 4 * (dem.shape[0] - 1), 4 * (dem.shape[1] - 1)
        s.drape(np.broadcast_to(np.array([0.6, 0.6, 0.6], f32), (rows, cols, 3)))
        texel = spacing / 4.0
        assert s.paint_contours(s.contour_levels(2.0, 0.5), rgba=(0.2, 0.1, 0.0, 0.8), width=1.5 * texel) > 0
        thin = s.paint_streams(3, rgba=(0.1, 0.3, 0.8, 1.0), width=1.5 * texel)
        trunk = s.paint_streams(12, rgba=(0.1, 0.3, 0.8, 1.0), width=3.0 * texel)
        assert thin > trunk > 0
        by_hand = s.render()
    _same(got, by_hand, "contours, then streams and their trunks")
    v.disable_streams()
    v.disable_contours()
    _same(v.render(), plain, "streams disabled")
