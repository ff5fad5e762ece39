"""Vector features painted onto the drape of a live session (f3d_session_paint), on the device.

* the device returns the bits of the host build of the lane body (tests/paint_host: every primitive for every texel, no tiles),
  read back through drape_image(): canvases 1x1, 7x9, 16x16, 70x130 and 257x64 over a 33x33 DEM at 10 m and an anisotropic
  33x17 one at (10, 7) m, registrations "area", "point" and one with a negative scale_z; per canvas points, then lines, then
  triangles over each other, with primitives across tile edges and more of them over one tile than two LDS chunks hold;
* the same with vertices out to the contract's reach (2^16 texels from the terrain's centre); one beyond it is refused;
* a painted session renders, bit for bit, what a fresh session draped with the first one's drape_image() renders -- with and
  without a mesh, after frames were already enqueued (the paint restarts the render), after reaim, rearm and reterrain;
* a strip session paints the whole canvas;
* every refusal leaves fingerprint() and drape_image() as they were;
* ViewerHandle with two vector layers renders what the equivalent drape + paint calls render.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_session_drape_host import CAM, drape_dem, drape_kw, random_image, unpack
from test_session_paint_host import (ANISO, CASES, KINDS, SQUARE, case_content, f32, far_content, flipped, frame_of, harness, host_paint,  # noqa: F401
                                     random_canvas, records)

pytestmark = pytest.mark.gpu

W, H = 64, 48
AOVS = ("rgba", "albedo", "normal", "depth")
ORBIT = {"origin": (63.6, 45.0, 63.6), "look_at": (0.0, 5.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or CAM), **opts, **kw)


def _frames(s, n=2):
    s.enqueue_frames(0, n)
    return s.resolve(n)


def _same(got, want, what):
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key}"


def _bits(image):
    return np.ascontiguousarray(image, f32).view(np.uint32)


@pytest.fixture(scope="module")
def sessions():
    """One session per DEM of the canvas cases (the canvases and registrations change per case, through drape())."""
    out = {}
    for dem_shape, spacing in (SQUARE, ANISO):
        dem = drape_dem(dem_shape)
        out[dem_shape] = _session(dem, dict(drape_kw(dem), spacing=spacing))
    yield out
    for s in out.values():
        s.close()


@pytest.mark.parametrize("canvas,dem,kind", CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_the_device_returns_the_bits_of_the_host_body(harness, sessions, canvas, dem, kind):  # noqa: F811
    dem_shape, spacing = dem
    s = sessions[dem_shape]
    reg = flipped(dem_shape, canvas) if kind == "flipped" else s.drape_registration(canvas[0], canvas[1], kind)
    frame = frame_of(dem_shape, spacing, reg)
    image = np.random.default_rng(3).uniform(0.05, 0.95, (*canvas, 3)).astype(f32)
    s.drape(image, registration=tuple(float(v) for v in reg), filter="nearest")
    texels = random_canvas(canvas, 3)
    assert np.array_equal(_bits(s.drape_image()), _bits(unpack(texels))), "drape_image() returns what the texels hold"
    for n, prim in enumerate(("points", "lines", "triangles")):
        xz, rgba, idx, feat, width = case_content(prim, canvas, frame, 20 + n)
        opacity = (0.7, 1.0, 0.45)[n]
        s.paint(xz, rgba, idx, primitive=prim, width=width, opacity=opacity, features=feat)
        hw = float(f32(width) * f32(0.5))
        want = host_paint(harness, texels, frame, records(xz, rgba, idx, KINDS[prim], feat), KINDS[prim], hw, opacity)
        got = s.drape_image()
        wrong = int((_bits(got) != _bits(unpack(want))).any(-1).sum())
        assert wrong == 0, f"{prim} on {canvas}: {wrong} of {want.size} texels differ from the host body"
        assert (want != texels).any(), prim
        texels = want
    if canvas[0] >= 16 and canvas[1] >= 16:  # a region of it
        assert np.array_equal(_bits(s.drape_image((3, 5, 9, 7))), _bits(unpack(texels)[3:12, 5:12]))


@pytest.mark.parametrize("canvas,dem,kind", [CASES[3], CASES[4]], ids=["square-70x130", "aniso-257x64-flipped"])
def test_vertices_out_to_the_reach_give_the_host_bits_and_beyond_it_are_refused(harness, sessions, canvas, dem, kind):  # noqa: F811
    dem_shape, spacing = dem
    s = sessions[dem_shape]
    reg = flipped(dem_shape, canvas) if kind == "flipped" else s.drape_registration(canvas[0], canvas[1], kind)
    frame = frame_of(dem_shape, spacing, reg)
    s.drape(np.random.default_rng(14).uniform(0.05, 0.95, (*canvas, 3)).astype(f32), registration=tuple(float(v) for v in reg))
    texels = random_canvas(canvas, 14)
    for n, prim in enumerate(("lines", "triangles")):
        xz, rgba, idx, feat, width = far_content(prim, canvas, frame, 60 + n)
        s.paint(xz, rgba, idx, primitive=prim, width=width, opacity=0.8, features=feat)
        want = host_paint(harness, texels, frame, records(xz, rgba, idx, KINDS[prim], feat), KINDS[prim], float(f32(width) * f32(0.5)), 0.8)
        assert np.array_equal(_bits(s.drape_image()), _bits(unpack(want))), prim
        assert (want != texels).sum() > 100, prim
        texels = want
    one = float(max(abs(frame[2] / frame[4]), abs(frame[3] / frame[6])))
    before = s.fingerprint(), s.drape_image().tobytes()
    with pytest.raises(RuntimeError, match="paint vertices lie more than 65536 texels"):
        s.paint(np.array([[0.0, 0.0], [65537.0 * one, 0.0]], f32), (1, 0, 0))
    assert (s.fingerprint(), s.drape_image().tobytes()) == before
    s.paint(np.array([[0.0, 0.0], [0.0, -65535.0 * one]], f32), (1, 0, 0), width=2.0 * one)  # (inside the reach: painted)
    assert s.drape_image().tobytes() != before[1]


def _paint_some(s, seed=1):
    """Three calls of three kinds over the session's drape, features and opacity included."""
    rng = np.random.default_rng(seed)
    span = 0.5 * scenes.SPAN
    road = np.stack([np.linspace(-span, span, 9), 0.4 * span * np.sin(np.linspace(0, 5, 9))], 1).astype(f32)
    s.paint(road, (0.9, 0.8, 0.1, 1.0), primitive="lines", width=4.0, opacity=0.8)
    quad = np.array([[-0.6, -0.5], [0.1, -0.6], [0.2, 0.3], [-0.5, 0.4]], f32) * f32(span)
    s.paint(quad, np.array([[0.1, 0.6, 0.2, 0.9]] * 4, f32), [0, 1, 2, 0, 2, 3], primitive="triangles", opacity=0.5)
    peaks = rng.uniform(-span, span, (12, 2)).astype(f32)
    s.paint(peaks, rng.uniform(0, 1, (12, 4)).astype(f32), primitive="points", width=6.0, features=np.arange(12))


@pytest.mark.parametrize("mesh", [False, True], ids=["terrain", "mesh"])
def test_a_painted_session_renders_what_a_session_draped_with_its_canvas_renders(mesh):
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2, mesh=mesh)
    image = random_image((48, 80), 71)
    with _session(dem, kw) as s:
        s.drape(image)
        before = s.drape_image()
        s.enqueue_frames(0, 1)  # (frames in flight over the old canvas: the paint is ordered behind them and restarts the render)
        _paint_some(s)
        canvas = s.drape_image()
        assert (canvas != before).any(-1).mean() > 0.05
        got = _frames(s)
    with _session(dem, kw) as fresh:
        fresh.drape(canvas)
        assert np.array_equal(_bits(fresh.drape_image()), _bits(canvas)), "binary16 values go through drape() unchanged"
        want = _frames(fresh)
    _same(got, want, "painted")
    with _session(dem, kw) as plain:
        plain.drape(image)
        assert not np.array_equal(_frames(plain)["albedo"], got["albedo"]), "the paint is visible"


def test_a_painted_canvas_survives_the_other_updates():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    dem2 = (dem * f32(0.8) + f32(0.1)).astype(f32)
    steps = [("rearm", lambda s: s.rearm(sun_azimuth_deg=80.0, seed=11), dict(kw, sun_azimuth_deg=80.0, seed=11), dem, CAM),
             ("reaim", lambda s: s.reaim(ORBIT), dict(kw, sun_azimuth_deg=80.0, seed=11), dem, ORBIT),
             ("reterrain", lambda s: s.reterrain(dem2), dict(kw, sun_azimuth_deg=80.0, seed=11), dem2, ORBIT)]
    with _session(dem, kw) as s:
        s.drape(random_image((40, 40), 72), filter="nearest")
        _paint_some(s, 2)
        canvas = s.drape_image()
        for name, update, fresh_kw, fresh_dem, cam in steps:
            update(s)
            assert np.array_equal(_bits(s.drape_image()), _bits(canvas)), name
            got = _frames(s)
            with _session(fresh_dem, fresh_kw, cam=cam) as fresh:
                fresh.drape(canvas, filter="nearest")
                _same(got, _frames(fresh), f"after {name}")
        # and a paint is an update itself: camera and re-armable values ride along
        s.paint(np.array([[0.0, 0.0]], f32), (1.0, 0.0, 0.0), primitive="points", width=30.0, camera=CAM, seed=5)
        final = s.drape_image()
        got = _frames(s)
        with _session(dem2, dict(kw, sun_azimuth_deg=80.0, seed=5), cam=CAM) as fresh:
            fresh.drape(final, filter="nearest")
            _same(got, _frames(fresh), "paint with a camera and a seed")


def test_a_strip_session_paints_the_whole_canvas(harness):  # noqa: F811
    dem_shape, spacing = SQUARE
    dem = drape_dem(dem_shape)
    canvas = (70, 130)
    with _session(dem, dict(drape_kw(dem), spacing=spacing), row_begin=16, row_end=32) as s:
        reg = s.drape_registration(canvas[0], canvas[1], "area")
        frame = frame_of(dem_shape, spacing, reg)
        s.drape(np.random.default_rng(3).uniform(0.05, 0.95, (*canvas, 3)).astype(f32))
        texels = random_canvas(canvas, 3)
        xz, rgba, idx, feat, width = case_content("lines", canvas, frame, 31)
        s.paint(xz, rgba, idx, primitive="lines", width=width, opacity=0.6, features=feat)
        want = host_paint(harness, texels, frame, records(xz, rgba, idx, 1, feat), 1, float(f32(width) * f32(0.5)), 0.6)
        assert np.array_equal(_bits(s.drape_image()), _bits(unpack(want)))
        assert (want != texels).mean() > 0.2


def _raw(s, xz, rgba, indices, primitive=1, half_width=2.0, opacity=1.0, **members):
    """f3d_session_paint with a descriptor of the caller's: (status, message)."""
    from forge3d_amd import _native

    xz, rgba, indices = np.ascontiguousarray(xz, f32), np.ascontiguousarray(rgba, f32), np.ascontiguousarray(indices, np.uint32)
    q = _native.PaintDesc()
    q.struct_size = C.sizeof(_native.PaintDesc)
    q.primitive, q.vertex_count = primitive, len(xz)
    q.xz, q.rgba, q.indices, q.index_count = xz.ctypes.data, rgba.ctypes.data, indices.ctypes.data, indices.size
    q.half_width, q.opacity = half_width, opacity
    q.aim = s._aim(None, {})
    for k, v in members.items():
        setattr(q, k, v)
    err = C.create_string_buffer(1024)
    rc = s._lib.f3d_session_paint(s._handle, C.byref(q), err, len(err))
    return rc, err.value.decode()


def test_every_refusal_leaves_the_session_and_the_canvas_as_they_were():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    xz = np.array([[-20, -20], [20, -10], [0, 25]], f32)
    red = np.array([[1, 0, 0, 1]] * 3, f32)
    with _session(dem, kw) as s:
        fp = s.fingerprint()
        assert _raw(s, xz, red, [0, 1]) == (1, "this session has no drape: vector features are painted into one (f3d_session_drape gives the canvas)")
        with pytest.raises(ValueError, match="this session has no drape"):
            s.paint(xz, (1, 0, 0))
        with pytest.raises(ValueError, match="no drape to read"):
            s.drape_image()
        assert s.fingerprint() == fp and not s.draped
        s.drape(random_image((24, 40), 73))
        s.enqueue_frames(0, 1)
        state = lambda: (s.fingerprint(), s.info()["gpu_resource_bytes"], s.drape_info(), s.drape_image().tobytes())  # noqa: E731
        before = state()
        bad = xz.copy()
        bad[1, 0] = np.nan
        pale = red.copy()
        pale[2, 3] = 1.5
        for what, call, status, text in (
                ("an index >= N", lambda: _raw(s, xz, red, [0, 3]), 1, "paint index 1 is 3, the call has 3 vertices"),
                ("an odd index count", lambda: _raw(s, xz, red, [0, 1, 2]), 1, "3 indices do not make line segments"),
                ("no indices", lambda: _raw(s, xz, red, [0, 1], index_count=0), 1, "0 indices do not make"),
                ("an unknown primitive", lambda: _raw(s, xz, red, [0, 1], primitive=3), 1, "paint primitive must be 0 (points), 1 (lines) or 2 (triangles), got 3"),
                ("an unknown flag", lambda: _raw(s, xz, red, [0, 1], flags=4), 1, "unknown paint flags 0x4"),
                ("a negative width", lambda: _raw(s, xz, red, [0, 1], half_width=-1.0), 1, "paint half_width must be finite and >= 0"),
                ("a NaN width", lambda: _raw(s, xz, red, [0, 1], half_width=float("nan")), 1, "paint half_width must be finite and >= 0"),
                ("an opacity above 1", lambda: _raw(s, xz, red, [0, 1], opacity=1.25), 1, "paint opacity must lie in [0, 1]"),
                ("a wrong struct size", lambda: _raw(s, xz, red, [0, 1], struct_size=8), 1, "f3d_session_paint_desc.struct_size is 8"),
                ("a NaN vertex", lambda: _raw(s, bad, red, [0, 1]), 3, "paint vertices contain non-finite coordinates"),
                ("an alpha above 1", lambda: _raw(s, xz, pale, [0, 1]), 3, "paint colours must lie in [0, 1]")):
            rc, message = call()
            assert rc == status and text in message, (what, rc, message)
            assert state() == before, what
        with pytest.raises(RuntimeError, match="paint vertices contain non-finite coordinates"):
            s.paint(bad, (1, 0, 0))
        assert state() == before
        region = (C.c_uint32 * 4)(20, 0, 10, 10)
        out = np.zeros((10, 10, 3), f32)
        assert s._lib.f3d_session_drape_read(s._handle, region, out.ctypes.data, s._err, len(s._err)) == 1 and b"leaves the session's 24x40 drape" in s._err.value
        # what is accepted after all that paints, and removing the drape gives the paint's buffers back
        s.paint(xz, (1, 0, 0), [0, 1, 2], primitive="triangles")
        assert state()[3] != before[3] and s.info()["gpu_resource_bytes"] > before[1]
        s.drape(None)
        assert s.fingerprint()["drape"] == fp["drape"]
    with _session(dem, kw) as s:
        never = s.info()["gpu_resource_bytes"]
        s.drape(random_image((24, 40), 73))
        s.paint(xz, (1, 0, 0), [0, 1, 2], primitive="triangles")
        s.drape(None)
        assert s.info()["gpu_resource_bytes"] <= never + 8 * 2 ** 20, "the canvas and the paint's buffers went back (the upload slab aside)"


def test_a_paint_past_the_memory_budget_is_refused_and_the_canvas_stays():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    image = random_image((64, 64), 74)
    rng = np.random.default_rng(8)
    many = rng.uniform(-40, 40, (6000, 2)).astype(f32)  # 2000 triangles: 160 KB of records
    with _session(dem, kw) as s:
        s.drape(image)
        need = s.info()["gpu_resource_bytes"]
    with _session(dem, kw, memory_budget_bytes=need + 65536) as s:
        s.drape(image)
        s.paint(many[:30], (0, 0, 1), primitive="triangles")  # (a small call fits)
        before = s.fingerprint(), s.info()["gpu_resource_bytes"], s.drape_image().tobytes()
        with pytest.raises(RuntimeError, match="paint exceeds the memory budget"):
            s.paint(many, (1, 0, 0), primitive="triangles")
        assert (s.fingerprint(), s.info()["gpu_resource_bytes"], s.drape_image().tobytes()) == before
        # the keys: few records, every one over every tile of a larger canvas
    with _session(dem, kw) as s:
        s.drape(random_image((512, 512), 75))
        need = s.info()["gpu_resource_bytes"]
    with _session(dem, kw, memory_budget_bytes=need + 65536) as s:
        s.drape(random_image((512, 512), 75))
        span = 0.45 * scenes.SPAN
        big = np.tile(np.array([[-span, -span], [span, -span], [0, span]], f32), (40, 1))  # 40 triangles x ~1000 tiles x 16 B of keys
        s.enqueue_frames(0, 1)
        before = s.fingerprint(), s.drape_info(), s.drape_image().tobytes()
        with pytest.raises(RuntimeError, match="paint exceeds the memory budget: the \\(tile, primitive\\) keys"):
            s.paint(big, (1, 0, 0), primitive="triangles")
        # (the records' buffer had grown before the keys were counted: gpu_resource_bytes may have; nothing a render reads has)
        assert (s.fingerprint(), s.drape_info(), s.drape_image().tobytes()) == before


def test_vector_layers_render_what_the_equivalent_drape_and_paint_calls_render(tmp_path):
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
    parcel = [[x, 0.0, z, 0.2, 0.7, 0.3, 0.8, 4] for x, z in ((-span, -span), (span, -span), (-span, span), (span, span))]
    road = [[x, 50.0, 0.3 * span * np.sin(x / 9.0), 0.9, 0.1, 0.1, 1.0, 9] for x in np.linspace(-span, span, 7)]
    b = v.add_vector_overlay("road", road, list(range(7)), "line_strip", line_width=3.0, z_order=2)
    a = v.add_vector_overlay("parcel", parcel, [0, 1, 2, 3], "triangle_strip", opacity=0.6, z_order=1)
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
            xz = np.array([[r[0], r[2]] for r in parcel], f32)
            s.paint(xz, np.array([r[3:7] for r in parcel], f32), [0, 1, 2, 2, 1, 3], primitive="triangles", opacity=0.6, features=[4] * 4)
            xz = np.array([[r[0], r[2]] for r in road], f32)
            s.paint(xz, np.array([r[3:7] for r in road], f32), primitive="lines", width=3.0 * texel, features=[9] * 7)
            return s.render()

    _same(got, by_hand(), "two layers over the constant canvas")
    # over a loaded overlay image the layers are painted into it
    image = random_image((24, 40), 76)
    v.load_overlay("ortho", image, filter="nearest")
    _same(v.render(), by_hand(image, ViewerHandle.overlay_registration(dem.shape, image.shape, (0.0, 0.0, 1.0, 1.0))), "two layers over an overlay")
    v.render_animation([key], tmp_path / "frames")
    assert np.array_equal(f3d_io.png_to_numpy(tmp_path / "frames" / "frame_0000.png"), v.last_result["rgba"])
    v.remove_overlay("ortho")
    v.remove_vector_overlay(a)
    v.remove_vector_overlay(b)
    _same(v.render(), plain, "layers removed")
