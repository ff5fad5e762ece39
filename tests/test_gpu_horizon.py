"""Horizon rasters on a live terrain session (f3d_session_horizon; TerrainSession.horizon / sky_view_factor) on the device.

* the device against the host build of the same lane body (tests/horizon_host), bit for bit, planes and sky_view, on the CPU
  suite's shapes (5x3, 33x33, 64x64, 65x63): host form, device-tensor form, NO_WAIT, curved and flat, regions, NaN azimuths;
* the bracket against code that is already tested: visibility() along (dx_k, s, dz_k) equals `s > H_k` wherever
  |s - H_k| > 1e-3 (1 + |H_k|), -inf counted as lit, with at most 2 % of the samples left out per slope;
* after a reterrain with no host wait, a fresh session's planes; a session with a mesh answers as one without; a strip
  session answers the whole DEM; fingerprint() and a render with horizon calls interleaved are unchanged;
* the host scratch only grows; a call past memory_budget_bytes is refused and the session still renders; every refusal
  carries its message and leaves the render as it was.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_gpu_reaim import H, W, _same
from test_session_horizon_host import SLOPES, HostScene, azimuth_set, compass, f32, harness, left_out, shaped  # noqa: F401
from test_session_raster_host import SHAPES, _kw

pytestmark = pytest.mark.gpu


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or scenes.CAM), **opts, **kw)


def _city():
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    return dem, verts, tris, _kw(dem, mesh_vertices=verts, mesh_indices=tris)


def _bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_library_exports_the_horizon():
    from forge3d_amd import _native

    assert _native.lib().f3d_session_horizon is not None and _native.lib().f3d_abi_version() == 6


# ---- 1. device against the host build of the lane body ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_the_host_body_bit_for_bit(shaped, shape):  # noqa: F811
    import torch

    scene = shaped[shape]
    with _session(scene.dem, scene.kw) as s:
        for curved in (False, True):
            want = scene.run(compass(16), 1e-3, curved)
            assert not np.isnan(want["horizon"]).any()
            planes, sky = s.horizon(16, curved=curved, sky_view=True)
            assert planes.dtype == f32 and planes.shape == (16, *shape) and sky.dtype == f32 and sky.shape == shape
            assert _bits(planes, want["horizon"]) and _bits(sky, want["sky_view"]), f"host form, curved={curved}"
            assert _bits(s.horizon(16, curved=curved), want["horizon"]) and _bits(s.sky_view_factor(16, curved=curved), want["sky_view"])
            az = azimuth_set("three")
            want = scene.run(az, 0.5, curved)
            assert _bits(s.horizon(az, lift=0.5, curved=curved), want["horizon"]), "a (K, 2) array, used as given"
            d = torch.from_numpy(az).cuda()
            planes, sky = s.horizon(d, lift=0.5, curved=curved, sky_view=True)
            assert planes.is_cuda and sky.is_cuda and planes.dtype == torch.float32
            assert _bits(planes.cpu().numpy(), want["horizon"]) and _bits(sky.cpu().numpy(), want["sky_view"]), "device form"
            assert _bits(s.sky_view_factor(d, lift=0.5, curved=curved).cpu().numpy(), want["sky_view"]), "device form, horizon null"
            later = s.horizon(d, lift=0.5, curved=curved, sky_view=True, wait=False)  # NO_WAIT: in flight on the null stream
            torch.cuda.current_stream().synchronize()
            assert _bits(later[0].cpu().numpy(), want["horizon"]) and _bits(later[1].cpu().numpy(), want["sky_view"]), "device form, no wait"


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65)])
def test_regions_are_windows_of_the_whole_raster(shaped, region):  # noqa: F811
    scene = shaped[(63, 65)]
    want = scene.run(azimuth_set("one"), 0.5, True)
    r0, c0, r, c = region
    with _session(scene.dem, scene.kw) as s:
        planes, sky = s.horizon(azimuth_set("one"), lift=0.5, curved=True, region=region, sky_view=True)
        assert _bits(planes, want["horizon"][:, r0:r0 + r, c0:c0 + c]) and _bits(sky, want["sky_view"][r0:r0 + r, c0:c0 + c])


def test_nan_azimuths_in_the_tensor_form_answer_nan(shaped):  # noqa: F811
    import torch

    scene = shaped[(33, 33)]
    good = azimuth_set("one")[0]
    with _session(scene.dem, scene.kw) as s:
        for bad in ([np.nan, 1.0], [1.0, np.inf], [0.0, 0.0]):
            az = np.array([good, bad, good], f32)
            want = scene.run(az, 1e-3)
            planes, sky = s.horizon(torch.from_numpy(az).cuda(), sky_view=True)
            assert _bits(planes.cpu().numpy(), want["horizon"]) and _bits(sky.cpu().numpy(), want["sky_view"])
            assert np.isnan(want["horizon"][1]).all() and not np.isnan(want["horizon"][[0, 2]]).any() and not np.isnan(want["sky_view"]).any()
            with pytest.raises(ValueError, match="azimuth 1 is not a finite, non-zero"):
                s.horizon(az)


# ---- 2. the bracket against visibility() ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 33), (63, 65)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_horizon_brackets_visibility(shaped, shape):  # noqa: F811
    """`(dx_k, s, dz_k)` is lit exactly where s > H_k: the any-hit march of the visibility rasters, flat, terrain only, the
    same lift.  Within 1e-3 (1 + |H_k|) of the horizon the march's own rounding may decide; those samples are left out, and
    may be at most 2 % per slope."""
    scene = shaped[shape]
    az = compass(16)
    with _session(scene.dem, scene.kw) as s:
        h = s.horizon(16, lift=1e-3)
        assert not np.isnan(h).any()
        for slope in SLOPES:
            directions = np.stack([az[:, 0], np.full(16, slope, f32), az[:, 1]], 1).astype(f32)
            lit = s.visibility(directions, toward=False, curved=False, terrain_only=True, lift=1e-3)
            out = left_out(h.astype(np.float64), slope)
            share = float(out.mean())
            wrong = (lit != (slope > h)) & ~out
            print(f"{shape[1]}x{shape[0]} slope {slope}: lit {lit.mean():.3f}, left out {100 * share:.2f} %, wrong {int(wrong.sum())}")
            assert share <= 0.02, f"slope {slope}: {100 * share:.2f} % of the samples lie within the band"
            assert not wrong.any(), f"slope {slope}: {int(wrong.sum())} samples disagree with visibility(), first at {np.argwhere(wrong)[0]}"


# ---- 3. .. 6. the session around it -----------------------------------------------------------------------------------------------
def test_horizons_follow_reterrain_without_a_wait_and_ignore_the_mesh():
    dem, verts, tris, kw = _city()
    bare = _kw(dem)
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(np.float32)
    result = dem.copy()
    result[20:36, 20:36] = patch
    with _session(dem, kw) as s:
        before = s.horizon(16, sky_view=True)
        s.reterrain(patch, at=(20, 20))
        after = s.horizon(16, sky_view=True)
    with _session(dem, bare) as plain:
        got = plain.horizon(16, sky_view=True)
        assert _bits(before[0], got[0]) and _bits(before[1], got[1]), "a session with a mesh answers as one without"
    with _session(result, bare) as fresh:
        got = fresh.horizon(16, sky_view=True)
        assert _bits(after[0], got[0]) and _bits(after[1], got[1]), "after reterrain"
    assert (before[0] != after[0]).any() and (before[1] != after[1]).any()


def test_a_strip_session_answers_the_whole_dem(shaped):  # noqa: F811
    scene = shaped[(63, 65)]
    want = scene.run(compass(16), 1e-3, True)
    with _session(scene.dem, scene.kw, row_begin=16, row_end=40) as s:
        planes, sky = s.horizon(16, curved=True, sky_view=True)
        assert _bits(planes, want["horizon"]) and _bits(sky, want["sky_view"])


def test_horizons_change_nothing_a_frame_reads():
    dem, _, _, kw = _city()
    with _session(dem, kw) as s, _session(dem, kw) as plain:
        fp = s.fingerprint()
        s.horizon(16), s.sky_view_factor(8, curved=True), s.horizon(azimuth_set("three"), lift=0.5, region=(3, 4, 20, 21))
        assert s.fingerprint() == fp
        n = 4
        for f in range(n):
            s.enqueue_frames(f, 1, f + 1 == n)
            s.sky_view_factor(16, region=(f, 2 * f, 33, 40))
            s.horizon(4, curved=True)
            plain.enqueue_frames(f, 1, f + 1 == n)
        got, want = s.resolve(n), plain.resolve(n)
        for k in ("rgba", "albedo", "normal", "depth"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.window_stats() == plain.window_stats()


# ---- 7. memory -----------------------------------------------------------------------------------------------------------------
def test_the_host_scratch_only_grows_and_the_tensor_form_takes_nothing(shaped):  # noqa: F811
    import torch

    scene = shaped[(63, 65)]
    n = 63 * 65
    room = lambda b: (b + 15) & ~15
    with _session(scene.dem, scene.kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        s.horizon(torch.from_numpy(compass(16)).cuda(), sky_view=True)
        assert s.info()["gpu_resource_bytes"] == bytes0, "the device form takes nothing"
        s.sky_view_factor(16)
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * n) + 16 * 8, "sky_view and the azimuths: nothing of size K n"
        s.horizon(3)
        grown = s.info()["gpu_resource_bytes"]
        assert grown == bytes0 + room(3 * 4 * n) + 3 * 8, "a larger call grows it, the old one goes back"
        s.horizon(3), s.horizon(2, sky_view=True), s.sky_view_factor(16), s.shadow_mask()
        assert s.info()["gpu_resource_bytes"] == grown, "a repeated or smaller call, a visibility raster included, reuses the scratch"


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(s, azimuths, flags=0, region=(0, 0, 64, 64), lift=1e-3, struct_size=None, horizon=True, sky=False, reserved=0, k=None):
    from forge3d_amd import _native

    q = _native.HorizonDesc()
    q.struct_size = C.sizeof(_native.HorizonDesc) if struct_size is None else struct_size
    q.flags, q.lift, q.reserved = flags, lift, reserved
    q.row0, q.col0, q.rows, q.cols = region
    q.azimuth_count = (0 if azimuths is None else len(azimuths)) if k is None else k
    q.azimuths = None if azimuths is None else azimuths.ctypes.data
    n = min(max(q.rows * q.cols, 1), 64 * 64)  # (a call that is refused is refused before anything is written)
    h = np.zeros((min(max(q.azimuth_count, 1), 256), n), f32)
    v = np.zeros(n, f32)
    q.horizon, q.sky_view = (h.ctypes.data if horizon else None), (v.ctypes.data if sky else None)
    s._check(s._lib.f3d_session_horizon(s._handle, C.byref(q), s._err, len(s._err)))
    return h, v


def test_refusals_leave_the_session_rendering_what_it_rendered():
    dem, _, _, kw = _city()
    kw = scenes.fixed_frames(kw, 4)
    az = np.ascontiguousarray(compass(16))
    scratch = 16 * 4 * 64 * 64 + 4 * 64 * 64 + 16 * 8  # planes, sky_view, azimuths (more than a create's own transient peak)
    with _session(dem, kw) as probe:
        need = probe.info()["gpu_resource_bytes"] + scratch
        want = probe.render()
    with _session(dem, kw, memory_budget_bytes=need - 1) as s:
        fp = s.fingerprint()
        for match, call in (
                ("struct_size", lambda: _raw(s, az, struct_size=16)),
                ("unknown horizon flags", lambda: _raw(s, az, flags=1)),
                ("unknown horizon flags", lambda: _raw(s, az, flags=16)),
                ("reserved", lambda: _raw(s, az, reserved=1)),
                ("NO_WAIT needs DEVICE_POINTERS", lambda: _raw(s, az, flags=8)),
                ("outside the 64x64 DEM", lambda: _raw(s, az, region=(0, 1, 64, 64))),
                ("outside the 64x64 DEM", lambda: _raw(s, az, region=(64, 0, 1, 1))),
                ("outside the 64x64 DEM", lambda: _raw(s, az, region=(1, 0, 0xFFFFFFFF, 1))),
                ("empty horizon region", lambda: _raw(s, az, region=(0, 0, 0, 64))),
                ("empty horizon region", lambda: _raw(s, az, region=(3, 3, 5, 0))),
                ("lift must be finite and not negative", lambda: _raw(s, az, lift=float("nan"))),
                ("lift must be finite and not negative", lambda: _raw(s, az, lift=float("inf"))),
                ("lift must be finite and not negative", lambda: _raw(s, az, lift=-1e-3)),
                ("1 to 256 azimuths, got 0", lambda: _raw(s, az[:0])),
                ("1 to 256 azimuths, got 257", lambda: _raw(s, az, k=257)),
                ("null azimuths", lambda: _raw(s, None, k=2)),
                ("both null", lambda: _raw(s, az, horizon=False)),
                ("azimuth 1 is not a finite, non-zero", lambda: _raw(s, np.array([[0, 1], [0, np.nan]], f32))),
                ("azimuth 0 is not a finite, non-zero", lambda: _raw(s, np.array([[np.inf, 1]], f32))),
                ("azimuth 2 is not a finite, non-zero", lambda: _raw(s, np.array([[0, 1], [1, 0], [0, 0]], f32)))):
            with pytest.raises(ValueError, match=match):
                call()
            # (what a frame launch reads is what it read: the render that follows this refusal is the render before it)
            assert s.fingerprint() == fp and s.info()["gpu_resource_bytes"] == need - scratch, f"after the refusal '{match}'"
        with pytest.raises(RuntimeError, match="memory budget"):
            s.horizon(16, sky_view=True)
        assert s.info()["gpu_resource_bytes"] == need - scratch and s.fingerprint() == fp
        assert s.horizon(15, sky_view=True)[0].shape == (15, 64, 64), "one azimuth fewer fits"
        assert s.sky_view_factor(256).shape == (64, 64), "with horizon null nothing of size K n is taken"
        _same(s.render(), {k: v for k, v in want.items() if k != "gpu_resource_bytes"}, "after the refusals")
    with _session(dem, kw, memory_budget_bytes=need) as s:
        assert s.horizon(16, sky_view=True)[0].shape == (16, 64, 64), "the budget that fits"
        with pytest.raises(ValueError, match="wait=False"):
            s.horizon(16, wait=False)
        with pytest.raises(ValueError, match="must not be negative"):
            s.horizon(16, region=(0, -1, 4, 4))
        h, v = _raw(s, az[:1], sky=True)
        assert np.isfinite(v).all() and (h != 0).any()
