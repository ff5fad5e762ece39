"""Shadow-depth rasters on a live terrain session (f3d_session_umbra; TerrainSession.umbra / lit_height) on the device.

* the device against the host build of the same lane body (tests/umbra_host), bit for bit, planes and `deepest`, on the CPU
  suite's shapes (5x3, 33x33, 64x64, 65x63) and its ten directions: host form, device-tensor form, NO_WAIT, curved and flat,
  (K, 3) input, regions, bad directions, the session's sun;
* the bracket against code that is already tested: visibility(d, toward=False, lift=rung, terrain_only=True) equals
  `rung > L*` wherever |rung - L*| > 2e-3 (1 + L* + |h| + relief), with at most 4 % of the samples left out per rung and none
  wrong; shadow_mask() one-sided at its own bias; the sun-hours count at lift 3 against the count of planes below 3;
* after a reterrain with no host wait, a fresh session's planes; a session with a mesh answers as one without; a strip
  session answers the whole DEM; fingerprint() and a render with umbra calls interleaved are unchanged; the session's sun
  follows rearm();
* the host scratch only grows and is the other raster families'; a call past memory_budget_bytes is refused and the session
  still renders; every refusal carries its message, in the contract's order, and leaves the render as it was.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_gpu_reaim import H, W, _same
from test_session_raster_host import SHAPES, _kw, sun_direction
from test_session_umbra_host import BAND, NAMES, RUNGS, WALKED, HostScene, directions, f32, harness, shaped  # noqa: F401

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


def test_the_library_exports_the_umbra():
    from forge3d_amd import _native

    assert _native.lib().f3d_session_umbra is not None and _native.lib().f3d_abi_version() == 6


# ---- 1. device against the host build of the lane body ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_the_host_body_bit_for_bit(shaped, shape):  # noqa: F811
    import torch

    scene = shaped[shape]
    dirs = directions(scene)
    with _session(scene.dem, scene.kw) as s:
        for curved in (False, True):
            want = scene.run(dirs, curved)
            assert not np.isnan(want["depth"]).any()
            planes, deep = s.umbra(dirs, curved=curved, deepest=True)
            assert planes.dtype == f32 and planes.shape == (10, *shape) and deep.dtype == f32 and deep.shape == shape
            assert _bits(planes, want["depth"]) and _bits(deep, want["deepest"]), f"host form, curved={curved}"
            assert _bits(s.umbra(dirs, curved=curved), want["depth"]), "host form, deepest null"
            assert _bits(s.umbra(dirs, curved=curved, planes=False, deepest=True), want["deepest"]), "host form, depth null"
            assert _bits(s.umbra(dirs[:, :3], curved=curved), want["depth"]), "(K, 3): the fourth is 0"
            d = torch.from_numpy(dirs).cuda()
            planes, deep = s.umbra(d, curved=curved, deepest=True)
            assert planes.is_cuda and deep.is_cuda and planes.dtype == torch.float32
            assert _bits(planes.cpu().numpy(), want["depth"]) and _bits(deep.cpu().numpy(), want["deepest"]), "device form"
            assert _bits(s.umbra(d, curved=curved).cpu().numpy(), want["depth"]), "device form, deepest null"
            assert _bits(s.umbra(d, curved=curved, planes=False, deepest=True).cpu().numpy(), want["deepest"]), "device form, depth null"
            assert _bits(s.umbra(d[:, :3], curved=curved).cpu().numpy(), want["depth"]), "device form, (K, 3)"
            later = s.umbra(d, curved=curved, deepest=True, wait=False)  # NO_WAIT: in flight on the null stream
            torch.cuda.current_stream().synchronize()
            assert _bits(later[0].cpu().numpy(), want["depth"]) and _bits(later[1].cpu().numpy(), want["deepest"]), "device form, no wait"
            sun = scene.run(None, curved)
            assert _bits(s.umbra(None, curved=curved, deepest=True)[0], sun["depth"]), "the session's sun"
            assert _bits(s.lit_height(curved=curved), sun["depth"][0])


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (62, 0, 1, 65), (31, 0, 1, 65), (20, 20, 1, 1)])
def test_regions_are_windows_of_the_whole_raster(shaped, region):  # noqa: F811
    scene = shaped[(63, 65)]
    dirs = directions(scene)
    want = scene.run(dirs, True)
    r0, c0, r, c = region
    with _session(scene.dem, scene.kw) as s:
        planes, deep = s.umbra(dirs, curved=True, region=region, deepest=True)
        assert _bits(planes, want["depth"][:, r0:r0 + r, c0:c0 + c]) and _bits(deep, want["deepest"][r0:r0 + r, c0:c0 + c])
        assert _bits(s.lit_height(dirs[0, :3], region=region), want["depth"][0, r0:r0 + r, c0:c0 + c])


def test_bad_directions_in_the_tensor_form_answer_nan(shaped):  # noqa: F811
    import torch

    scene = shaped[(33, 33)]
    good = directions(scene)[1]
    with _session(scene.dem, scene.kw) as s:
        for bad in ([np.nan, good[1], good[2], 0.0], [good[0], np.inf, good[2], 0.0], [good[0], good[1], -np.inf, 0.0], [good[0], good[1], good[2], np.nan],
                    [0.0, 0.0, 0.0, 0.0], [good[0], good[1], good[2], 1.0]):
            d = np.stack([good, np.array(bad, f32), good])
            want = scene.run(d)
            planes, deep = s.umbra(torch.from_numpy(d).cuda(), curved=False, deepest=True)
            assert _bits(planes.cpu().numpy(), want["depth"]) and _bits(deep.cpu().numpy(), want["deepest"])
            assert np.isnan(want["depth"][1]).all() and not np.isnan(want["depth"][[0, 2]]).any() and not np.isnan(want["deepest"]).any()
            with pytest.raises(ValueError, match="umbra direction 1 is not a finite, non-zero"):
                s.umbra(d, curved=False)


# ---- 2. the bracket against visibility() ----------------------------------------------------------------------------------------
def _band(lstar, h, relief):
    return BAND * (1.0 + np.where(np.isfinite(lstar), lstar, 0.0) + np.abs(h) + relief)


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", [(33, 33), (63, 65)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_umbra_brackets_visibility(shaped, shape, curved):  # noqa: F811
    """A sample lifted by a rung is lit exactly where rung > L*: the any-hit march of the visibility rasters along the direction,
    terrain only, the same curvature flag.  Within 2e-3 (1 + L* + |h| + relief) of L* the march's own rounding may decide; those
    samples are left out, and may be at most 4 % per rung (tests/test_session_umbra_host.py: at most 2.74 % on the reference)."""
    scene = shaped[shape]
    dirs = directions(scene)[:5]
    h = scene.surface.h64
    with _session(scene.dem, scene.kw) as s:
        lstar = s.umbra(dirs, curved=curved).astype(np.float64)
        assert not np.isnan(lstar).any() and np.isfinite(lstar).all()
        for k in range(5):
            band = _band(lstar[k], h, scene.relief)
            for rung in RUNGS:
                lit = s.visibility(dirs[k:k + 1], toward=False, lift=rung, terrain_only=True, curved=curved)[0]
                out = np.abs(rung - lstar[k]) <= band
                share = float(out.mean())
                wrong = (lit != (rung > lstar[k])) & ~out
                print(f"{shape[1]}x{shape[0]} {NAMES[k]} rung {rung}: lit {lit.mean():.3f}, left out {100 * share:.2f} %, wrong {int(wrong.sum())}")
                assert share <= 0.04, f"rung {rung}: {100 * share:.2f} % of the samples lie within the band"
                assert not wrong.any(), f"rung {rung}: {int(wrong.sum())} samples disagree with visibility(), first at {np.argwhere(wrong)[0]}"


@pytest.mark.parametrize("shape", [(33, 33), (63, 65)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_lit_height_against_shadow_mask_and_sun_hours(shaped, shape):  # noqa: F811
    """One-sided at the shadow mask's own bias (the clamp puts every lit sample at exactly 0, inside any band): a sample whose L*
    lies above the bias by more than its band is in shadow in shadow_mask(d), and outside the band around the bias the mask is
    `lit_height < bias`; the count of track positions that light a sample lifted by 3 is the count of planes below 3 where no
    plane lies in its band, and differs from it by at most the number of planes that do."""
    from forge3d_amd.session import TerrainSession

    scene = shaped[shape]
    dirs = directions(scene)
    h = scene.surface.h64
    with _session(scene.dem, scene.kw) as s:
        for k in (0, 1, 3):
            d = dirs[k, :3]
            lh = s.lit_height(d)
            assert lh.dtype == f32 and lh.shape == shape and not np.isnan(lh).any() and (lh >= 0).all()
            assert _bits(lh, s.umbra(dirs[k:k + 1], curved=True)[0]), "lit_height is umbra's plane of the direction, curved"
            lstar = lh.astype(np.float64)
            band = _band(lstar, h, scene.relief)
            mask = s.shadow_mask(d, terrain_only=True)
            above = lstar > band + TerrainSession.SURFACE_BIAS
            assert above.any() and not mask[above].any(), "a sample that needs more than its band is in shadow at the ground"
            agree = mask == (lh < f32(TerrainSession.SURFACE_BIAS))
            out = np.abs(TerrainSession.SURFACE_BIAS - lstar) <= band
            print(f"{shape[1]}x{shape[0]} {NAMES[k]}: lit {mask.mean():.3f}, shadow_mask == (lit_height < bias) on {agree.mean():.4f}, in the band {out.mean():.3f}")
            assert agree[~out].all(), "the docstrings' identity, away from the band"
        track = np.stack([sun_direction(az, el)[:3] for az, el in ((300.0, 4.0), (315.0, 8.0), (330.0, 14.0), (345.0, 20.0), (10.0, 26.0), (90.0, -3.0))])
        up = track[track[:, 1] > 0]
        assert len(up) == 5
        planes, deep = s.umbra(up, curved=True, deepest=True)
        assert _bits(s.lit_height(track), deep), "a track: `deepest`, the positions below the horizontal dropped"
        assert _bits(deep, np.fmax.reduce(planes))
        lift = 3.0
        hours = s.visibility(up, toward=False, curved=True, terrain_only=True, lift=lift, masks=False, count=True)
        below = (planes < f32(lift)).sum(0)
        near = (np.abs(lift - planes.astype(np.float64)) <= _band(planes.astype(np.float64), h, scene.relief)).any(0)
        print(f"{shape[1]}x{shape[0]} sun hours at lift 3: mean {hours.mean():.3f} of 5, {100 * near.mean():.2f} % with a plane in its band")
        assert np.array_equal(hours[~near], below[~near].astype(hours.dtype)) and not near.all()
        assert (np.abs(hours.astype(np.int64) - below) <= (np.abs(lift - planes.astype(np.float64)) <= _band(planes.astype(np.float64), h, scene.relief)).sum(0)).all()
        assert (s.lit_height(track[5:]) == 0).all() and s.lit_height(track[5:], region=(1, 2, 3, 4)).shape == (3, 4), "an empty track: zeros"
        assert _bits(s.sun_hours(track, terrain_only=True), s.visibility(up, toward=False, curved=True, terrain_only=True, lift=f32(TerrainSession.SURFACE_BIAS), masks=False, count=True))


# ---- 3. .. 6. the session around it -----------------------------------------------------------------------------------------------
def _city_directions():
    return np.stack([sun_direction(315.0, 5.0), sun_direction(200.0, 12.0), np.array([1.0, 0.17, 0.0, 0.0], f32), np.array([0.6, -0.05, 0.8, 0.0], f32)]).astype(f32)


def test_umbras_follow_reterrain_without_a_wait_and_ignore_the_mesh():
    dem, verts, tris, kw = _city()
    bare = _kw(dem)
    dirs = _city_directions()
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(np.float32)
    result = dem.copy()
    result[20:36, 20:36] = patch
    with _session(dem, kw) as s:
        before = s.umbra(dirs, deepest=True)
        sun_before = s.umbra(None)
        s.reterrain(patch, at=(20, 20))
        after = s.umbra(dirs, deepest=True)
    with _session(dem, bare) as plain:
        got = plain.umbra(dirs, deepest=True)
        assert _bits(before[0], got[0]) and _bits(before[1], got[1]), "a session with a mesh answers as one without"
        assert _bits(sun_before, plain.umbra(None))
    with _session(result, bare) as fresh:
        got = fresh.umbra(dirs, deepest=True)
        assert _bits(after[0], got[0]) and _bits(after[1], got[1]), "after reterrain"
    assert (before[0] != after[0]).any() and (before[1] != after[1]).any()
    assert (before[0][0] > 0).any() and (before[0][0] == 0).any()


def test_a_strip_session_answers_the_whole_dem(shaped):  # noqa: F811
    scene = shaped[(63, 65)]
    dirs = directions(scene)
    want = scene.run(dirs, True)
    with _session(scene.dem, scene.kw, row_begin=16, row_end=40) as s:
        planes, deep = s.umbra(dirs, curved=True, deepest=True)
        assert _bits(planes, want["depth"]) and _bits(deep, want["deepest"])


def test_umbras_change_nothing_a_frame_reads():
    dem, _, _, kw = _city()
    dirs = _city_directions()
    with _session(dem, kw) as s, _session(dem, kw) as plain:
        fp = s.fingerprint()
        s.umbra(dirs), s.lit_height(dirs[:2, :3], curved=False), s.umbra(None, deepest=True, region=(3, 4, 20, 21))
        assert s.fingerprint() == fp
        n = 4
        for f in range(n):
            s.enqueue_frames(f, 1, f + 1 == n)
            s.lit_height(dirs[0, :3], region=(f, 2 * f, 33, 40))
            s.umbra(dirs, curved=True)
            plain.enqueue_frames(f, 1, f + 1 == n)
        got, want = s.resolve(n), plain.resolve(n)
        for k in ("rgba", "albedo", "normal", "depth"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.window_stats() == plain.window_stats()


def test_the_sessions_sun_follows_rearm(harness):  # noqa: F811
    dem = scenes.golden_dem(4)
    kw = _kw(dem)
    moved = {**kw, "sun_azimuth_deg": 100.0, "sun_elevation_deg": 9.0}
    first, second = HostScene(harness, dem, kw), HostScene(harness, dem, moved)
    try:
        with _session(dem, kw) as s:
            for curved in (True, False):
                assert _bits(s.umbra(None, curved=curved), first.run(None, curved)["depth"])
            s.rearm(sun_azimuth_deg=100.0, sun_elevation_deg=9.0)
            for curved in (True, False):
                got = s.umbra(None, curved=curved, deepest=True)
                want = second.run(None, curved)
                assert _bits(got[0], want["depth"]) and _bits(got[1], want["deepest"]), "the direction the frames' sun rays use now"
                assert _bits(got[0], s.umbra(np.array([[*second.sun, 0.0]], f32), curved=curved)), "the explicit direction"
            assert not _bits(first.run(None, True)["depth"], second.run(None, True)["depth"])
    finally:
        first.close()
        second.close()


# ---- 7. memory -----------------------------------------------------------------------------------------------------------------
def test_the_host_scratch_only_grows_and_the_tensor_form_takes_nothing(shaped):  # noqa: F811
    import torch

    scene = shaped[(63, 65)]
    dirs = directions(scene)
    n = 63 * 65
    room = lambda b: (b + 15) & ~15
    with _session(scene.dem, scene.kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        s.umbra(torch.from_numpy(dirs).cuda(), deepest=True)
        assert s.info()["gpu_resource_bytes"] == bytes0, "the device form takes nothing"
        s.umbra(None)
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * n), "the session's sun: one plane, no direction goes up"
        s.umbra(dirs, planes=False, deepest=True)
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * n) + 10 * 16, "deepest and the directions: nothing of size K n"
        s.umbra(dirs[:3])
        grown = s.info()["gpu_resource_bytes"]
        assert grown == bytes0 + room(3 * 4 * n) + 3 * 16, "a larger call grows it, the old one goes back"
        s.umbra(dirs[:3]), s.umbra(dirs[:2], deepest=True), s.lit_height(dirs[:5, :3]), s.shadow_mask()
        s.clearance(np.array([[0.0, 30.0, 0.0, 0.0]], f32)), s.horizon(2), s.irradiation(dirs[:2, :3], np.ones(2, f32))
        assert s.info()["gpu_resource_bytes"] == grown, "a repeated or smaller call of any raster family reuses the scratch"
        s.clearance(np.tile(np.array([[0.0, 30.0, 0.0, 0.0]], f32), (4, 1)))
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * 4 * n) + 4 * 16, "a larger clearance grows the same buffer"
        s.umbra(dirs[:4])
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * 4 * n) + 4 * 16


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(s, dirs, flags=0, region=(0, 0, 64, 64), struct_size=None, depth=True, deepest=False, reserved=0, k=None):
    from forge3d_amd import _native

    q = _native.UmbraDesc()
    q.struct_size = C.sizeof(_native.UmbraDesc) if struct_size is None else struct_size
    q.flags, q.reserved = flags, reserved
    q.row0, q.col0, q.rows, q.cols = region
    q.direction_count = (0 if dirs is None else len(dirs)) if k is None else k
    q.directions = None if dirs is None else dirs.ctypes.data
    n = min(max(q.rows * q.cols, 1), 64 * 64)  # (a call that is refused is refused before anything is written)
    p = np.zeros((max(q.direction_count, 1), n), f32)
    v = np.zeros(n, f32)
    q.depth, q.deepest = (p.ctypes.data if depth else None), (v.ctypes.data if deepest else None)
    s._check(s._lib.f3d_session_umbra(s._handle, C.byref(q), s._err, len(s._err)))
    return p, v


def test_refusals_leave_the_session_rendering_what_it_rendered():
    dem, _, _, kw = _city()
    kw = scenes.fixed_frames(kw, 4)
    rng = np.random.default_rng(11)
    d = np.ascontiguousarray(np.stack([rng.uniform(-1, 1, 16), rng.uniform(0.05, 0.5, 16), rng.uniform(-1, 1, 16), np.zeros(16)], 1), f32)
    scratch = 16 * 4 * 64 * 64 + 4 * 64 * 64 + 16 * 16  # planes, deepest, directions (more than a create's own transient peak)
    bad_region = (0, 1, 64, 64)
    with _session(dem, kw) as probe:
        need = probe.info()["gpu_resource_bytes"] + scratch
        want = probe.render()
    with _session(dem, kw, memory_budget_bytes=need - 1) as s:
        fp = s.fingerprint()
        for match, call in (
                ("struct_size", lambda: _raw(s, d, struct_size=16, flags=32)),
                ("unknown umbra flags", lambda: _raw(s, d, flags=1, reserved=1)),
                ("unknown umbra flags", lambda: _raw(s, d, flags=32)),
                ("reserved", lambda: _raw(s, d, reserved=1, flags=8)),
                ("NO_WAIT needs DEVICE_POINTERS", lambda: _raw(s, d, flags=8 | 16)),
                ("SESSION_SUN is the session's own sun direction: it takes no directions", lambda: _raw(s, d, flags=16, region=bad_region)),
                ("SESSION_SUN is the session's own sun direction: it takes no directions", lambda: _raw(s, None, flags=16, k=2)),
                ("outside the 64x64 DEM", lambda: _raw(s, d[:0], region=bad_region)),
                ("outside the 64x64 DEM", lambda: _raw(s, d, region=(64, 0, 1, 1))),
                ("outside the 64x64 DEM", lambda: _raw(s, None, flags=16, region=(1, 0, 0xFFFFFFFF, 1))),
                ("empty umbra region", lambda: _raw(s, d, region=(0, 0, 0, 64))),
                ("empty umbra region", lambda: _raw(s, d, region=(3, 3, 5, 0))),
                ("at least one direction", lambda: _raw(s, None, depth=False)),
                ("at least one direction", lambda: _raw(s, d[:0])),
                ("null directions", lambda: _raw(s, None, k=2, depth=False)),
                ("both null", lambda: _raw(s, np.array([[0, 0, 0, 0]], f32), depth=False)),
                ("both null", lambda: _raw(s, None, flags=16, depth=False)),
                ("umbra direction 1 is not a finite, non-zero", lambda: _raw(s, np.array([[0, 1, 1, 0], [0, np.nan, 0, 0]], f32))),
                ("umbra direction 0 is not a finite, non-zero", lambda: _raw(s, np.array([[np.inf, 1, 1, 0]], f32))),
                ("umbra direction 2 is not a finite, non-zero", lambda: _raw(s, np.array([[0, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0]], f32))),
                ("umbra direction 1 is not a finite, non-zero", lambda: _raw(s, np.array([[0, 1, 1, 0], [1, 1, 0, 0.5]], f32))),
                ("umbra direction 0 is not a finite, non-zero", lambda: _raw(s, np.array([[1, 1, 0, np.nan]], f32)))):
            with pytest.raises(ValueError, match=match):
                call()
            # (what a frame launch reads is what it read: the render that follows this refusal is the render before it)
            assert s.fingerprint() == fp and s.info()["gpu_resource_bytes"] == need - scratch, f"after the refusal '{match}'"
        with pytest.raises(RuntimeError, match="memory budget"):
            s.umbra(d, deepest=True)
        assert s.info()["gpu_resource_bytes"] == need - scratch and s.fingerprint() == fp
        assert s.umbra(d[:15], deepest=True)[0].shape == (15, 64, 64), "one direction fewer fits"
        assert s.umbra(np.tile(d, (16, 1)), planes=False, deepest=True).shape == (64, 64), "with depth null nothing of size K n is taken"
        _same(s.render(), {k: v for k, v in want.items() if k != "gpu_resource_bytes"}, "after the refusals")
    with _session(dem, kw, memory_budget_bytes=need) as s:
        assert s.umbra(d, deepest=True)[0].shape == (16, 64, 64), "the budget that fits"
        with pytest.raises(ValueError, match="wait=False"):
            s.umbra(d, wait=False)
        with pytest.raises(ValueError, match="wait=False"):
            s.umbra(None, wait=False)
        with pytest.raises(ValueError, match="must not be negative"):
            s.umbra(d, region=(0, -1, 4, 4))
        with pytest.raises(ValueError, match="needs an output"):
            s.umbra(d, planes=False)
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            s.lit_height(d)
        p, v = _raw(s, d[:1], deepest=True)
        assert _bits(p[0], v) and (p > 0).any() and (p == 0).any()
        p, _ = _raw(s, None, flags=16)
        assert _bits(p[0].reshape(64, 64), s.umbra(None, curved=False)[0]), "SESSION_SUN through the raw descriptor"
