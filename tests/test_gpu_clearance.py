"""Clearance rasters on a live terrain session (f3d_session_clearance; TerrainSession.clearance / visible_height) on the device.

* the device against the host build of the same lane body (tests/clearance_host), bit for bit, planes and `lowest`, on the
  CPU suite's shapes (5x3, 33x33, 64x64, 65x63) and its seven observers: host form, device-tensor form, NO_WAIT, curved and
  flat, regions, NaN observers;
* the bracket against code that is already tested: visibility(observer, toward=True, lift=L, terrain_only=True) equals
  `L > L*` wherever |L - L*| > 2e-3 (1 + |L*| + |Y| + h), with at most 2 % of the samples left out per rung; one-sided at
  the viewshed's own bias, and viewshed(target_height=3) against visible_height();
* after a reterrain with no host wait, a fresh session's planes; a session with a mesh answers as one without; a strip
  session answers the whole DEM; fingerprint() and a render with clearance calls interleaved are unchanged;
* the host scratch only grows; a call past memory_budget_bytes is refused and the session still renders; every refusal
  carries its message and leaves the render as it was.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_gpu_reaim import H, W, _same
from test_session_clearance_host import BAND, NAMES, RUNGS, HostScene, f32, harness, observers, shaped  # noqa: F401
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


def test_the_library_exports_the_clearance():
    from forge3d_amd import _native

    assert _native.lib().f3d_session_clearance is not None and _native.lib().f3d_abi_version() == 6


# ---- 1. device against the host build of the lane body ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_the_host_body_bit_for_bit(shaped, shape):  # noqa: F811
    import torch

    scene = shaped[shape]
    obs = observers(scene)
    with _session(scene.dem, scene.kw) as s:
        for curved in (False, True):
            want = scene.run(obs, curved)
            assert not np.isnan(want["height"]).any()
            planes, low = s.clearance(obs, curved=curved, lowest=True)
            assert planes.dtype == f32 and planes.shape == (7, *shape) and low.dtype == f32 and low.shape == shape
            assert _bits(planes, want["height"]) and _bits(low, want["lowest"]), f"host form, curved={curved}"
            assert _bits(s.clearance(obs, curved=curved), want["height"])
            assert _bits(s.clearance(obs, curved=curved, planes=False, lowest=True), want["lowest"]), "host form, height null"
            assert _bits(s.clearance(obs[:, :3], curved=curved)[[0, 2]], want["height"][[0, 2]]), "(K, 3): no distance limit"
            d = torch.from_numpy(obs).cuda()
            planes, low = s.clearance(d, curved=curved, lowest=True)
            assert planes.is_cuda and low.is_cuda and planes.dtype == torch.float32
            assert _bits(planes.cpu().numpy(), want["height"]) and _bits(low.cpu().numpy(), want["lowest"]), "device form"
            assert _bits(s.clearance(d, curved=curved, planes=False, lowest=True).cpu().numpy(), want["lowest"]), "device form, height null"
            later = s.clearance(d, curved=curved, lowest=True, wait=False)  # NO_WAIT: in flight on the null stream
            torch.cuda.current_stream().synchronize()
            assert _bits(later[0].cpu().numpy(), want["height"]) and _bits(later[1].cpu().numpy(), want["lowest"]), "device form, no wait"


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65), (20, 20, 1, 1)])
def test_regions_are_windows_of_the_whole_raster(shaped, region):  # noqa: F811
    scene = shaped[(63, 65)]
    obs = observers(scene)
    want = scene.run(obs, True)
    r0, c0, r, c = region
    with _session(scene.dem, scene.kw) as s:
        planes, low = s.clearance(obs, curved=True, region=region, lowest=True)
        assert _bits(planes, want["height"][:, r0:r0 + r, c0:c0 + c]) and _bits(low, want["lowest"][r0:r0 + r, c0:c0 + c])


def test_nan_observers_in_the_tensor_form_answer_nan(shaped):  # noqa: F811
    import torch

    scene = shaped[(33, 33)]
    good = observers(scene)[0]
    with _session(scene.dem, scene.kw) as s:
        for slot, value in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan)):
            bad = good.copy()
            bad[slot] = value
            ob = np.stack([good, bad, good])
            want = scene.run(ob)
            planes, low = s.clearance(torch.from_numpy(ob).cuda(), lowest=True)
            assert _bits(planes.cpu().numpy(), want["height"]) and _bits(low.cpu().numpy(), want["lowest"])
            assert np.isnan(want["height"][1]).all() and not np.isnan(want["height"][[0, 2]]).any() and not np.isnan(want["lowest"]).any()
            with pytest.raises(ValueError, match="observer 1 is not a finite"):
                s.clearance(ob)


# ---- 2. the bracket against visibility() ----------------------------------------------------------------------------------------
def _band(lstar, Y, h):
    return BAND * (1.0 + np.abs(np.where(np.isfinite(lstar), lstar, 0.0)) + abs(float(Y)) + h)


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", [(33, 33), (63, 65)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_clearance_brackets_visibility(shaped, shape, curved):  # noqa: F811
    """A sample lifted by L is seen exactly where L > L*: the any-hit march of the visibility rasters toward the observer,
    terrain only, the same curvature flag.  Within 2e-3 (1 + |L*| + |Y| + h) of L* the march's own rounding may decide; those
    samples are left out, and may be at most 2 % per rung."""
    scene = shaped[shape]
    obs = observers(scene)[:4]
    h = scene.surface.h64
    with _session(scene.dem, scene.kw) as s:
        lstar = s.clearance(obs, curved=curved).astype(np.float64)
        assert not np.isnan(lstar).any()
        for k in range(4):
            band = _band(lstar[k], obs[k, 1], h)
            for rung in RUNGS:
                seen = s.visibility(obs[k:k + 1], toward=True, lift=rung, terrain_only=True, curved=curved)[0]
                out = np.isfinite(lstar[k]) & (np.abs(rung - lstar[k]) <= band)
                share = float(out.mean())
                wrong = (seen != (rung > lstar[k])) & ~out
                print(f"{shape[1]}x{shape[0]} {NAMES[k]} rung {rung}: seen {seen.mean():.3f}, left out {100 * share:.2f} %, wrong {int(wrong.sum())}")
                assert share <= 0.02, f"rung {rung}: {100 * share:.2f} % of the samples lie within the band"
                assert not wrong.any(), f"rung {rung}: {int(wrong.sum())} samples disagree with visibility(), first at {np.argwhere(wrong)[0]}"


@pytest.mark.parametrize("shape", [(33, 33), (63, 65)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_visible_height_against_viewshed(shaped, shape):  # noqa: F811
    """One-sided at the viewshed's own bias (the clamp puts every visible sample at exactly 0, inside any band): a sample whose
    L* lies above its band is hidden in viewshed(obs); and viewshed(obs, target_height=3) is visible_height(obs) < 3 + 1e-3
    outside the band."""
    scene = shaped[shape]
    all_obs = observers(scene)
    h = scene.surface.h64
    with _session(scene.dem, scene.kw) as s:
        for k, limit in ((0, None), (3, None), (0, 0.35 * float(scene.spacing[0]) * (shape[1] - 1))):
            ob = all_obs[k, :3]
            vh = s.visible_height(ob, max_distance=limit)
            assert vh.dtype == f32 and vh.shape == shape and not np.isnan(vh).any() and (vh >= 0).all()
            want = s.clearance(np.array([[*ob, limit or 0.0]], f32))[0]
            assert _bits(vh, want), "visible_height is clearance's `lowest` of the observers"
            lstar = vh.astype(np.float64)
            band = _band(lstar, ob[1], h)
            ground = s.viewshed(ob, max_distance=limit, terrain_only=True)
            above = ~np.isfinite(lstar) | (lstar > band)
            assert above.any() and not ground[above].any(), "a sample that needs more than its band is hidden at the ground"
            th = 3.0
            raised = s.viewshed(ob, target_height=th, max_distance=limit, terrain_only=True)
            out = np.isfinite(lstar) & (np.abs(th + 1e-3 - lstar) <= band)
            wrong = (raised != (vh < f32(th + 1e-3))) & ~out
            print(f"{shape[1]}x{shape[0]} {NAMES[k]} limit {limit}: ground shows {ground.mean():.3f}, at 3 m {raised.mean():.3f}, left out {100 * out.mean():.2f} %")
            assert out.mean() <= 0.02 and not wrong.any()
        two = s.visible_height(all_obs[[0, 3], :3])
        assert _bits(two, np.fmin(s.visible_height(all_obs[0, :3]), s.visible_height(all_obs[3, :3]))), "several observers: seen by any"
        ox, oz = float(scene.origin[0]), float(scene.origin[1])
        standing = s.visible_height((0.3 * ox, 0.2 * oz))
        y = s.ground(np.array([[0.3 * ox, 0.2 * oz]], f32))[0] + f32(1.7)
        assert _bits(standing, s.visible_height((0.3 * ox, y, 0.2 * oz))), "(x, z): standing observer_height above ground()"
        nowhere = s.visible_height((3.0 * ox, 0.0))
        assert nowhere.shape == shape and np.isposinf(nowhere).all(), "no ground under the observer: nothing is ever seen"


# ---- 3. .. 6. the session around it -----------------------------------------------------------------------------------------------
def _city_observers():
    return np.array([[-15.0, 16.0, -10.0, 0.0], [10.0, 18.0, -5.0, 35.0], [70.0, 9.0, -15.0, 0.0]], f32)


def test_clearances_follow_reterrain_without_a_wait_and_ignore_the_mesh():
    dem, verts, tris, kw = _city()
    bare = _kw(dem)
    obs = _city_observers()
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(np.float32)
    result = dem.copy()
    result[20:36, 20:36] = patch
    with _session(dem, kw) as s:
        before = s.clearance(obs, lowest=True)
        s.reterrain(patch, at=(20, 20))
        after = s.clearance(obs, lowest=True)
    with _session(dem, bare) as plain:
        got = plain.clearance(obs, lowest=True)
        assert _bits(before[0], got[0]) and _bits(before[1], got[1]), "a session with a mesh answers as one without"
    with _session(result, bare) as fresh:
        got = fresh.clearance(obs, lowest=True)
        assert _bits(after[0], got[0]) and _bits(after[1], got[1]), "after reterrain"
    assert (before[0] != after[0]).any() and (before[1] != after[1]).any()
    assert (before[0][0] > 0).any() and (before[0][0] == 0).any() and np.isposinf(before[0][1]).any()


def test_a_strip_session_answers_the_whole_dem(shaped):  # noqa: F811
    scene = shaped[(63, 65)]
    obs = observers(scene)
    want = scene.run(obs, True)
    with _session(scene.dem, scene.kw, row_begin=16, row_end=40) as s:
        planes, low = s.clearance(obs, curved=True, lowest=True)
        assert _bits(planes, want["height"]) and _bits(low, want["lowest"])


def test_clearances_change_nothing_a_frame_reads():
    dem, _, _, kw = _city()
    obs = _city_observers()
    with _session(dem, kw) as s, _session(dem, kw) as plain:
        fp = s.fingerprint()
        s.clearance(obs), s.visible_height(obs[:, :3], curved=True), s.clearance(obs[:1], lowest=True, region=(3, 4, 20, 21))
        assert s.fingerprint() == fp
        n = 4
        for f in range(n):
            s.enqueue_frames(f, 1, f + 1 == n)
            s.visible_height(obs[0, :3], region=(f, 2 * f, 33, 40))
            s.clearance(obs, curved=True)
            plain.enqueue_frames(f, 1, f + 1 == n)
        got, want = s.resolve(n), plain.resolve(n)
        for k in ("rgba", "albedo", "normal", "depth"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.window_stats() == plain.window_stats()


# ---- 7. memory -----------------------------------------------------------------------------------------------------------------
def test_the_host_scratch_only_grows_and_the_tensor_form_takes_nothing(shaped):  # noqa: F811
    import torch

    scene = shaped[(63, 65)]
    obs = observers(scene)
    n = 63 * 65
    room = lambda b: (b + 15) & ~15
    with _session(scene.dem, scene.kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        s.clearance(torch.from_numpy(obs).cuda(), lowest=True)
        assert s.info()["gpu_resource_bytes"] == bytes0, "the device form takes nothing"
        s.clearance(obs, planes=False, lowest=True)
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * n) + 7 * 16, "lowest and the observers: nothing of size K n"
        s.clearance(obs[:3])
        grown = s.info()["gpu_resource_bytes"]
        assert grown == bytes0 + room(3 * 4 * n) + 3 * 16, "a larger call grows it, the old one goes back"
        s.clearance(obs[:3]), s.clearance(obs[:2], lowest=True), s.visible_height(obs[:, :3]), s.shadow_mask()
        assert s.info()["gpu_resource_bytes"] == grown, "a repeated or smaller call, a visibility raster included, reuses the scratch"


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(s, observers_, flags=0, region=(0, 0, 64, 64), struct_size=None, height=True, lowest=False, reserved=0, k=None):
    from forge3d_amd import _native

    q = _native.ClearanceDesc()
    q.struct_size = C.sizeof(_native.ClearanceDesc) if struct_size is None else struct_size
    q.flags, q.reserved = flags, reserved
    q.row0, q.col0, q.rows, q.cols = region
    q.observer_count = (0 if observers_ is None else len(observers_)) if k is None else k
    q.observers = None if observers_ is None else observers_.ctypes.data
    n = min(max(q.rows * q.cols, 1), 64 * 64)  # (a call that is refused is refused before anything is written)
    h = np.zeros((max(q.observer_count, 1), n), f32)
    v = np.zeros(n, f32)
    q.height, q.lowest = (h.ctypes.data if height else None), (v.ctypes.data if lowest else None)
    s._check(s._lib.f3d_session_clearance(s._handle, C.byref(q), s._err, len(s._err)))
    return h, v


def test_refusals_leave_the_session_rendering_what_it_rendered():
    dem, _, _, kw = _city()
    kw = scenes.fixed_frames(kw, 4)
    rng = np.random.default_rng(11)
    ob = np.ascontiguousarray(np.stack([rng.uniform(-40, 40, 16), rng.uniform(15, 25, 16), rng.uniform(-40, 40, 16), np.zeros(16)], 1), f32)
    scratch = 16 * 4 * 64 * 64 + 4 * 64 * 64 + 16 * 16  # planes, lowest, observers (more than a create's own transient peak)
    with _session(dem, kw) as probe:
        need = probe.info()["gpu_resource_bytes"] + scratch
        want = probe.render()
    with _session(dem, kw, memory_budget_bytes=need - 1) as s:
        fp = s.fingerprint()
        for match, call in (
                ("struct_size", lambda: _raw(s, ob, struct_size=16)),
                ("unknown clearance flags", lambda: _raw(s, ob, flags=1)),
                ("unknown clearance flags", lambda: _raw(s, ob, flags=16)),
                ("reserved", lambda: _raw(s, ob, reserved=1)),
                ("NO_WAIT needs DEVICE_POINTERS", lambda: _raw(s, ob, flags=8)),
                ("outside the 64x64 DEM", lambda: _raw(s, ob, region=(0, 1, 64, 64))),
                ("outside the 64x64 DEM", lambda: _raw(s, ob, region=(64, 0, 1, 1))),
                ("outside the 64x64 DEM", lambda: _raw(s, ob, region=(1, 0, 0xFFFFFFFF, 1))),
                ("empty clearance region", lambda: _raw(s, ob, region=(0, 0, 0, 64))),
                ("empty clearance region", lambda: _raw(s, ob, region=(3, 3, 5, 0))),
                ("at least one observer", lambda: _raw(s, ob[:0])),
                ("null observers", lambda: _raw(s, None, k=2)),
                ("both null", lambda: _raw(s, ob, height=False)),
                ("observer 1 is not a finite", lambda: _raw(s, np.array([[0, 20, 1, 0], [0, np.nan, 0, 0]], f32))),
                ("observer 0 is not a finite", lambda: _raw(s, np.array([[np.inf, 20, 1, 0]], f32))),
                ("observer 0 is not a finite", lambda: _raw(s, np.array([[0, 20, 1, np.inf]], f32))),
                ("observer 2 has a negative maximum distance", lambda: _raw(s, np.array([[0, 20, 1, 0], [1, 20, 0, 5], [0, 20, 0, -1]], f32)))):
            with pytest.raises(ValueError, match=match):
                call()
            # (what a frame launch reads is what it read: the render that follows this refusal is the render before it)
            assert s.fingerprint() == fp and s.info()["gpu_resource_bytes"] == need - scratch, f"after the refusal '{match}'"
        with pytest.raises(RuntimeError, match="memory budget"):
            s.clearance(ob, lowest=True)
        assert s.info()["gpu_resource_bytes"] == need - scratch and s.fingerprint() == fp
        assert s.clearance(ob[:15], lowest=True)[0].shape == (15, 64, 64), "one observer fewer fits"
        assert s.clearance(np.tile(ob, (16, 1)), planes=False, lowest=True).shape == (64, 64), "with height null nothing of size K n is taken"
        _same(s.render(), {k: v for k, v in want.items() if k != "gpu_resource_bytes"}, "after the refusals")
    with _session(dem, kw, memory_budget_bytes=need) as s:
        assert s.clearance(ob, lowest=True)[0].shape == (16, 64, 64), "the budget that fits"
        with pytest.raises(ValueError, match="wait=False"):
            s.clearance(ob, wait=False)
        with pytest.raises(ValueError, match="must not be negative"):
            s.clearance(ob, region=(0, -1, 4, 4))
        with pytest.raises(ValueError, match="needs an output"):
            s.clearance(ob, planes=False)
        with pytest.raises(ValueError, match="max_distance must be positive"):
            s.visible_height(ob[0, :3], max_distance=0.0)
        h, v = _raw(s, ob[:1], lowest=True)
        assert _bits(h[0], v) and (h > 0).any() and (h == 0).any()
