"""Contour lines on a live session (f3d_session_contours, f3d_session_paint_contours), on the device.

* contours() returns the bits of the host build of the lane bodies (tests/contour_host: count, scan, emit over whole waves) --
  segments and level indices, in order and in number -- for contour_cases' DEMs, regions and level lists;
* a capacity below the total returns the prefix and leaves guard words behind it untouched; the device form equals the host form;
* state that outlives a call: a large call, then a small one; after reterrain (whole, with at=, with a new exaggeration) the
  result is a fresh session's on the new DEM; a strip session returns the whole DEM's contours;
* paint_contours() leaves drape_image() bit-identical to a twin session that ran paint(contours()["segments"]) with the same
  style -- on the square canvas and on the flipped anisotropic canvas of the paint tests -- and the two render the same bits in
  every AOV, with and without a mesh, after frames were already enqueued; a call that finds no segment leaves the drape's bits;
* every refusal, in its order, with its message, leaves fingerprint() and drape_image() as they were;
* ViewerHandle.enable_contours renders what the equivalent drape, paint_contours and paint calls render.
Every render is 64x48 with two frames.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import contour_cases as cases
import scenes
from test_session_drape_host import CAM, drape_dem, drape_kw, random_image
from test_session_paint_host import ANISO, SQUARE, flipped

pytestmark = pytest.mark.gpu

W, H = cases.SIZE
AOVS = ("rgba", "albedo", "normal", "depth")
f32 = np.float32


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
    assert got["total"] == want["total"], what
    assert got["segments"].tobytes() == want["segments"].tobytes(), what
    assert np.array_equal(got["level_index"], want["level_index"]), what


@pytest.fixture(scope="module")
def harness():
    return cases.build_harness()


@pytest.mark.parametrize("exaggeration", cases.EXAGGERATIONS)
@pytest.mark.parametrize("shape,spacing", cases.SHAPES, ids=[f"{s[1]}x{s[0]}" for s, _ in cases.SHAPES])
def test_the_device_returns_the_bits_of_the_host_body(harness, shape, spacing, exaggeration):
    dem = cases.shaped_dem(shape)
    kw = cases.shape_kw(dem, spacing, exaggeration)
    host = cases.HostContours(harness, dem, kw)
    try:
        with _session(dem, kw) as s:
            lists = cases.level_lists(host.heights, steep=shape[0] * shape[1] <= 81)  # (the 65536 levels: 2x2 and 5x3, and 9x9 -- a level-3 band)
            segments = 0
            for rname, region in cases.regions(shape).items():
                for lname, levels in lists.items():
                    if lname == "maximum count" and rname != "whole":
                        continue
                    got = s.contours(levels, region=region)
                    _equal(got, host.run(levels, region), f"{rname}, {lname}")
                    assert np.array_equal(got["levels"], levels)
                    segments += got["total"]
            assert segments > 0
    finally:
        host.close()


def test_capacity_guard_words_and_the_device_form(harness):
    import torch

    shape, spacing = cases.SHAPES[6]
    dem = cases.shaped_dem(shape)
    kw = cases.shape_kw(dem, spacing, 2.5)
    host = cases.HostContours(harness, dem, kw)
    try:
        levels = cases.level_lists(host.heights, steep=False)["interval"]
        want = host.run(levels)
        n, cap = want["total"], want["total"] // 3
        assert cap > 64
        with _session(dem, kw) as s:
            from forge3d_amd import _native

            seg, idx = np.full((cap + 8, 4), 77.0, f32), np.full(cap + 8, 77, np.uint32)
            total = C.c_uint64(0)
            q = _native.ContoursDesc()
            q.struct_size = C.sizeof(q)
            q.row0, q.col0, q.rows, q.cols = 0, 0, shape[0] - 1, shape[1] - 1
            q.levels, q.level_count = levels.ctypes.data, levels.size
            q.segments, q.level_index, q.capacity, q.total = seg.ctypes.data, idx.ctypes.data, cap, C.addressof(total)
            assert s._lib.f3d_session_contours(s._handle, C.byref(q), s._err, len(s._err)) == 0, s._err.value
            assert total.value == n and seg[:cap].tobytes() == want["segments"][:cap].tobytes() and np.array_equal(idx[:cap], want["level_index"][:cap])
            assert (seg[cap:] == 77.0).all() and (idx[cap:] == 77).all(), "guard words behind the capacity are untouched"
            # a generous capacity costs nothing: the scratch holds the records written, min(total, capacity), not the capacity
            held = s.info()["gpu_resource_bytes"]
            roomy, roomy_idx = np.full((n + 8, 4), 77.0, f32), np.full(n + 8, 77, np.uint32)
            q.segments, q.level_index, q.capacity = roomy.ctypes.data, roomy_idx.ctypes.data, 1 << 34  # (20 B a record: 320 GiB)
            assert s._lib.f3d_session_contours(s._handle, C.byref(q), s._err, len(s._err)) == 0, s._err.value
            assert total.value == n and roomy[:n].tobytes() == want["segments"].tobytes() and (roomy[n:] == 77.0).all()
            assert np.array_equal(roomy_idx[:n], want["level_index"])
            assert s.info()["gpu_resource_bytes"] - held <= 20 * n + 4096
            device = torch.device("cuda", torch.cuda.current_device())
            for room in (n + 5, cap):
                d_seg = torch.full((room + 8, 4), 77.0, dtype=torch.float32, device=device)
                d_idx = torch.full((room + 8,), 77, dtype=torch.int32, device=device)
                got = s.contours(levels, out=(d_seg[:room], d_idx[:room]))
                k = min(n, room)
                assert got["total"] == n and tuple(got["segments"].shape) == (k, 4)
                assert got["segments"].cpu().numpy().tobytes() == want["segments"][:k].tobytes()
                assert np.array_equal(got["level_index"].cpu().numpy().view(np.uint32), want["level_index"][:k])
                assert bool((d_seg[k:] == 77.0).all()) and bool((d_idx[k:] == 77).all())
            only = s.contours(levels, out=(torch.empty((n, 4), dtype=torch.float32, device=device), None))
            assert only["level_index"] is None and only["segments"].cpu().numpy().tobytes() == want["segments"].tobytes()
            chained = s.contours(levels, chain=True)
            assert sum(len(p["points"]) - 1 for p in chained["polylines"]) == n - int((want["segments"][:, :2] == want["segments"][:, 2:]).all(1).sum())
    finally:
        host.close()


def test_state_that_outlives_a_call(harness):
    """A large call, then a small one; reterrain whole, with at=, with a new exaggeration: always a fresh session's result."""
    shape, spacing = cases.SHAPES[6]
    dem = cases.shaped_dem(shape)
    kw = cases.shape_kw(dem, spacing, 2.5)

    def fresh(d, k, levels, region=None):
        host = cases.HostContours(harness, d, k)
        try:
            return host.run(levels, region), host.heights
        finally:
            host.close()

    with _session(dem, kw) as s:
        heights = fresh(dem, kw, np.array([1.0], f32))[1]
        lists = cases.level_lists(heights, steep=False)
        big = np.unique(np.linspace(heights.min(), heights.max(), 400).astype(f32))
        _equal(s.contours(big), fresh(dem, kw, big)[0], "a large call")
        _equal(s.contours(lists["one"], region=(5, 3, 13, 15)), fresh(dem, kw, lists["one"], (5, 3, 13, 15))[0], "then a small one")
        dem2 = (dem * f32(0.7) + f32(0.2) * np.roll(dem, 5, 1)).astype(f32)
        s.reterrain(dem2)
        _equal(s.contours(lists["interval"]), fresh(dem2, kw, lists["interval"])[0], "after reterrain")
        patch = (dem2[10:31, 20:45] + f32(0.3)).astype(f32)
        dem3 = dem2.copy()
        dem3[10:31, 20:45] = patch
        s.reterrain(patch, at=(10, 20))
        _equal(s.contours(lists["interval"]), fresh(dem3, kw, lists["interval"])[0], "after reterrain at=")
        s.reterrain(dem3, exaggeration=1.0)
        kw1 = dict(kw, exaggeration=1.0)
        small = (lists["interval"] / f32(2.5)).astype(f32)
        _equal(s.contours(small), fresh(dem3, kw1, small)[0], "after reterrain with a new exaggeration")
        assert s.contours(interval=float(small[1] - small[0]))["total"] > 0


def test_a_strip_session_returns_the_whole_dems_contours(harness):
    shape, spacing = cases.SHAPES[4]
    dem = cases.shaped_dem(shape)
    kw = cases.shape_kw(dem, spacing, 2.5)
    host = cases.HostContours(harness, dem, kw)
    try:
        levels = cases.level_lists(host.heights, steep=False)["interval"]
        with _session(dem, kw, row_begin=16, row_end=32) as s:
            _equal(s.contours(levels), host.run(levels), "strip")
    finally:
        host.close()


def _canvas(s, dem_shape, canvas, kind, seed):
    reg = flipped(dem_shape, canvas) if kind == "flipped" else s.drape_registration(canvas[0], canvas[1], kind)
    s.drape(random_image(canvas, seed), registration=tuple(float(v) for v in reg), filter="nearest")


@pytest.mark.parametrize("dem_case,canvas,kind", [(SQUARE, (70, 130), "area"), (ANISO, (257, 64), "flipped")], ids=["square-70x130", "aniso-257x64-flipped"])
def test_paint_contours_leaves_the_bits_of_the_host_route(dem_case, canvas, kind):
    dem_shape, spacing = dem_case
    dem = drape_dem(dem_shape)
    kw = dict(drape_kw(dem), spacing=spacing)
    style = dict(rgba=(0.1, 0.05, 0.0, 0.8), width=1.7 * spacing[0] * (dem_shape[1] - 1) / canvas[1], opacity=0.9)
    with _session(dem, kw) as a, _session(dem, kw) as b:
        _canvas(a, dem_shape, canvas, kind, 81)
        _canvas(b, dem_shape, canvas, kind, 81)
        before = a.drape_image()
        levels = a.contour_levels(2.0, base=0.5)
        for region in (None, (3, 2, 9, 11)):
            n = a.paint_contours(levels, region=region, **style)
            got = b.contours(levels, region=region)
            assert n == got["total"] > (50 if region is None else 10)
            b.paint(got["segments"].reshape(-1, 2), style["rgba"], primitive="lines", indices=np.arange(2 * n, dtype=np.uint32), width=style["width"],
                    opacity=style["opacity"])
            painted = a.drape_image()
            assert painted.tobytes() == b.drape_image().tobytes(), region
        assert (painted != before).any(-1).mean() > 0.05, "the lines are visible"
        assert a.paint_contours([1e6], **style) == 0 and a.drape_image().tobytes() == painted.tobytes(), "no segment: the drape keeps its bits"
        assert a.paint_stats()["primitives"] == n


@pytest.mark.parametrize("mesh", [False, True], ids=["terrain", "mesh"])
def test_the_two_routes_render_the_same_bits(mesh):
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2, mesh=mesh)
    image = random_image((48, 80), 82)
    with _session(dem, kw) as a, _session(dem, kw) as b, _session(dem, kw) as plain:
        for s in (a, b, plain):
            s.drape(image)
        a.enqueue_frames(0, 1)  # (frames in flight over the old canvas: the paint is ordered behind them and restarts the render)
        n = a.paint_contours(interval=2.5, width=1.5, rgba=(0.0, 0.0, 0.0, 0.8))
        got = b.contours(interval=2.5)
        assert n == got["total"] > 100
        b.paint(got["segments"].reshape(-1, 2), (0.0, 0.0, 0.0, 0.8), primitive="lines", indices=np.arange(2 * n, dtype=np.uint32), width=1.5)
        assert a.drape_image().tobytes() == b.drape_image().tobytes()
        assert a.fingerprint() == b.fingerprint()
        fa = _frames(a)
        _same(fa, _frames(b), "paint_contours against contours + paint")
        assert not np.array_equal(fa["albedo"], _frames(plain)["albedo"]), "the contours are visible"


def _raw(s, paint, levels, /, **members):
    """f3d_session_contours / f3d_session_paint_contours with a descriptor of the caller's: (status, message, total)."""
    from forge3d_amd import _native

    lv = np.ascontiguousarray(levels, f32)
    total = C.c_uint64(99)
    q = _native.PaintContoursDesc() if paint else _native.ContoursDesc()
    q.struct_size = C.sizeof(q)
    q.row0, q.col0, q.rows, q.cols = 0, 0, s.dem_shape[0] - 1, s.dem_shape[1] - 1
    q.levels, q.level_count, q.total = lv.ctypes.data, lv.size, C.addressof(total)
    if paint:
        q.rgba = (C.c_float * 4)(0.0, 0.0, 0.0, 0.8)
        q.half_width, q.opacity = 1.0, 1.0
        q.aim = s._aim(None, {})
    for k, v in members.items():
        setattr(q, k, v)
    err = C.create_string_buffer(1024)
    entry = s._lib.f3d_session_paint_contours if paint else s._lib.f3d_session_contours
    rc = entry(s._handle, C.byref(q), err, len(err))
    return rc, err.value.decode(), int(total.value)


def test_every_refusal_in_its_order_leaves_the_session_and_the_canvas_as_they_were():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    cell_h, cell_w = dem.shape[0] - 1, dem.shape[1] - 1
    nan, inf = float("nan"), float("inf")
    ok = [5.0, 10.0]
    shared = [
        ("the struct size", ok, dict(struct_size=8), 1, ".struct_size is 8"),
        ("unknown flags", ok, dict(flags=64), 1, "unknown contour flags 0x40"),
        ("reserved", ok, dict(reserved=3), 1, "reserved member must be 0, got 3"),
        ("an empty region", ok, dict(rows=0), 1, "empty contour region: 0 rows"),
        ("a region outside the cell grid", ok, dict(row0=cell_h), 1, f"lies outside the {cell_h}x{cell_w} cell grid"),
        ("a region one column too wide", ok, dict(col0=1), 1, f"lies outside the {cell_h}x{cell_w} cell grid"),
        ("null levels", ok, dict(levels=None), 1, "contour levels are empty"),
        ("no levels", ok, dict(level_count=0), 1, "contour levels are empty"),
        ("too many levels", ok, dict(level_count=65537), 1, "at most 65536 levels, got 65537"),
        ("a NaN level", [5.0, nan], {}, 1, "contour level 1 is not finite"),
        ("an infinite level", [inf], {}, 1, "contour level 0 is not finite"),
        ("levels not ascending", [5.0, 5.0], {}, 1, "strictly ascending: level 1 is 5 after 5"),
        ("a null total", ok, dict(total=None), 1, "null total"),
    ]
    with _session(dem, kw) as s:
        fp = s.fingerprint()
        rc, message, _ = _raw(s, True, ok)
        assert rc == 1 and message == "this session has no drape: contour lines are painted into one (f3d_session_drape gives the canvas)"
        with pytest.raises(ValueError, match="this session has no drape"):
            s.paint_contours(ok)
        assert s.fingerprint() == fp and not s.draped
        assert _raw(s, False, ok)[0] == 0, "the query needs no drape"
        s.drape(random_image((24, 40), 83))
        s.enqueue_frames(0, 1)
        state = lambda: (s.fingerprint(), s.drape_info(), s.drape_image().tobytes())  # noqa: E731
        before = state()
        for paint in (False, True):
            for what, levels, members, status, text in shared:
                rc, message, total = _raw(s, paint, levels, **members)
                assert rc == status and text in message, (paint, what, rc, message)
                assert total == 99 and state() == before, (paint, what)
            # the order: of two causes the earlier one's message wins
            for levels, members, text in (
                    (ok, dict(struct_size=8, flags=64), ".struct_size is 8"), (ok, dict(flags=64, reserved=3), "unknown contour flags"),
                    (ok, dict(reserved=3, rows=0), "reserved member"), (ok, dict(rows=0, row0=cell_h), "empty contour region"),
                    (ok, dict(row0=cell_h, level_count=0), "lies outside"), (ok, dict(levels=None, level_count=65537), "contour levels are empty"),
                    ([nan, 1.0], dict(level_count=65537), "at most 65536 levels"), ([5.0, 5.0], dict(total=None), "strictly ascending")):
                rc, message, _ = _raw(s, paint, levels, **members)
                assert rc == 1 and text in message, (paint, members, message)
            assert state() == before
        rc, message, _ = _raw(s, True, ok, total=None, half_width=-1.0)
        assert "null total" in message, "the shared checks come before the paint's own"
        seg = np.zeros((4, 4), f32)
        rc, message, _ = _raw(s, False, ok, capacity=4)
        assert rc == 1 and "null segments for a contour call with room for 4" in message
        rc, _, total = _raw(s, False, ok, segments=seg.ctypes.data, capacity=0)
        assert rc == 0 and total > 0 and not seg.any(), "a non-null output with capacity 0 is legal"
        rc, message, _ = _raw(s, False, ok, flags=4, segments=8, capacity=4)
        assert rc == 1 and "16-byte aligned" in message
        own = [
            ("a negative width", dict(half_width=-1.0), 1, "paint half_width must be finite and >= 0"),
            ("a NaN width", dict(half_width=nan), 1, "paint half_width must be finite and >= 0"),
            ("an opacity above 1", dict(opacity=1.25), 1, "paint opacity must lie in [0, 1]"),
            ("an alpha above 1", dict(rgba=(C.c_float * 4)(0.0, 0.0, 0.0, 1.5)), 3, "paint colours must lie in [0, 1]"),
            ("a NaN colour", dict(rgba=(C.c_float * 4)(nan, 0.0, 0.0, 1.0)), 3, "paint colours must lie in [0, 1]"),
        ]
        for what, members, status, text in own:
            rc, message, total = _raw(s, True, ok, **members)
            assert rc == status and text in message, (what, rc, message)
            assert total == 99 and state() == before, what
        rc, message, _ = _raw(s, True, ok, half_width=-1.0, opacity=2.0, rgba=(C.c_float * 4)(2.0, 0.0, 0.0, 1.0))
        assert "half_width" in message, "half_width, then opacity, then rgba"
        rc, message, _ = _raw(s, True, ok, opacity=2.0, rgba=(C.c_float * 4)(2.0, 0.0, 0.0, 1.0))
        assert "opacity" in message
        with pytest.raises(ValueError, match="strictly ascending"):
            s.paint_contours([3.0, 2.0])
        assert state() == before
        assert s.paint_contours(interval=5.0) > 0 and state()[2] != before[2], "what is accepted after all that paints"
    # the reach: a canvas so fine that the DEM's corner lies more than 2^16 texels from the centre
    with _session(dem, kw) as s:
        s.drape(random_image((8, 8), 84), registration=(4200.0, -0.5, 4200.0, -0.5), filter="nearest")
        before = s.fingerprint(), s.drape_image().tobytes()
        rc, message, total = _raw(s, True, ok)
        assert rc == 3 and "the contour region reaches more than 65536 texels of the drape" in message and total == 99
        assert (s.fingerprint(), s.drape_image().tobytes()) == before
        rc, _, _ = _raw(s, True, ok, row0=14, col0=14, rows=4, cols=4)
        assert rc == 0, "a region near the centre is inside the reach"


def test_too_many_segments_for_one_paint_call_are_refused_after_the_count():
    """More than F3D_PAINT_MAX_PRIMITIVES segments are only known after the count pass: every cell of a 65 x 65 sawtooth crosses
    all 65536 levels, 2^28 segments.  The canvas and the fingerprint stay; contours() still answers the total."""
    dem = np.tile((np.arange(65) % 2).astype(f32) * f32(64000.0), (65, 1))
    kw = cases.shape_kw(dem, (10.0, 10.0), 1.0)
    levels = np.unique(np.linspace(1.0, 63999.0, 65536).astype(f32))
    assert len(levels) == 65536
    with _session(dem, kw) as s:
        s.drape(random_image((16, 16), 85))
        before = s.fingerprint(), s.drape_image().tobytes()
        with pytest.raises(ValueError, match="a paint call takes at most 16777216 primitives, the contours have 268435456 segments"):
            s.paint_contours(levels)
        assert (s.fingerprint(), s.drape_image().tobytes()) == before
        rc, _, total = _raw(s, False, levels)
        assert rc == 0 and total == 64 * 64 * 65536


def test_enable_contours_renders_what_the_equivalent_calls_render(tmp_path):
    from forge3d_amd import io as f3d_io
    from forge3d_amd.session import TerrainSession
    from forge3d_amd.viewer import ViewerHandle

    dem = drape_dem()
    v = ViewerHandle(W, H, spp=2, max_frames=2, min_frames=2, variance_threshold=1e30)
    spacing = scenes.SPAN / (dem.shape[1] - 1)
    v.load_terrain(dem, spacing)
    v.set_z_scale(scenes.RELIEF)
    key = dict(phi_deg=28.0, theta_deg=49.0, radius=120.0, fov_deg=60.0)
    v.set_orbit_camera(**key)
    plain = v.render()
    span = 0.4 * scenes.SPAN
    road = [[x, 50.0, 0.3 * span * np.sin(x / 9.0), 0.9, 0.1, 0.1, 1.0, 9] for x in np.linspace(-span, span, 7)]
    v.enable_contours(2.0, base=0.5, width=1.5, rgba=(0.2, 0.1, 0.0, 0.8), index_every=5, index_width=3.0)
    layer = v.add_vector_overlay("road", road, list(range(7)), "line_strip", line_width=3.0)
    got = v.render()
    assert not np.array_equal(got["albedo"], plain["albedo"])

    def by_hand(image=None, reg=None):
        d, w, h, camera, keywords = v._call()
        with TerrainSession(d, w, h, camera, **keywords) as s:
            if image is None:
                rows, cols = 4 * (dem.shape[0] - 1), 4 * (dem.shape[1] - 1)
                s.drape(np.broadcast_to(np.array([0.6, 0.6, 0.6], f32), (rows, cols, 3)))
                texel = spacing / 4.0
            else:
                s.drape(image, registration=reg, filter="nearest")
                texel = max(abs(spacing / reg[0]), abs(spacing / reg[2]))
            levels = s.contour_levels(2.0, 0.5)
            assert s.paint_contours(levels, rgba=(0.2, 0.1, 0.0, 0.8), width=1.5 * texel) > 0
            k = np.rint((levels.astype(np.float64) - 0.5) / 2.0).astype(np.int64)
            assert s.paint_contours(levels[k % 5 == 0], rgba=(0.2, 0.1, 0.0, 0.8), width=3.0 * texel) > 0
            xz = np.array([[r[0], r[2]] for r in road], f32)
            s.paint(xz, np.array([r[3:7] for r in road], f32), primitive="lines", width=3.0 * texel, features=[9] * 7)
            return s.render()

    _same(got, by_hand(), "contours and a layer over the constant canvas")
    image = random_image((24, 40), 86)
    v.load_overlay("ortho", image, filter="nearest")
    _same(v.render(), by_hand(image, ViewerHandle.overlay_registration(dem.shape, image.shape, (0.0, 0.0, 1.0, 1.0))), "over an overlay")
    v.render_animation([key], tmp_path / "frames")
    assert np.array_equal(f3d_io.png_to_numpy(tmp_path / "frames" / "frame_0000.png"), v.last_result["rgba"])
    v.remove_overlay("ortho")
    v.remove_vector_overlay(layer)
    v.disable_contours()
    _same(v.render(), plain, "contours disabled")
