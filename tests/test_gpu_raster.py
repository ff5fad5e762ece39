"""DEM visibility rasters on a live terrain session (f3d_session_raster; TerrainSession.visibility / viewshed / shadow_mask /
sun_hours) on the device.

* the device against the oracle, bit for bit, on the CPU suite's shapes (tests/test_session_raster_host.py: 5x3, 33x33, 64x64,
  65x63; both target kinds; curved on and off; K = 1, 2, 3; a distance limit; the observer on a lifted sample; regions), in the
  host form and the device-tensor form, NO_WAIT included; NaN targets in the tensor form answer 0;
* the box city: masks equal session.occluded() of the same NumPy-built rays, with and without terrain_only, mesh builders 0, 2, 3;
* SESSION_SUN equals the armed direction; after rearm / reterrain / remesh, with no host wait in between, a fresh session's;
* a strip session answers the whole DEM; fingerprint() and a render with raster calls interleaved are unchanged;
* the host scratch only grows; a call past memory_budget_bytes is refused and the session still renders; every refusal
  carries its message and leaves the render as it was;
* the reference's curved-earth golden: IoU >= 0.98 curved, the flat control below.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_gpu_reaim import H, W, _same
from test_session_raster_host import (ALONG, SHAPES, TOWARD, HostScene, _kw, contract_bits, contract_origins, contract_rays, f32,  # noqa: F401
                                      harness, iou, shaped, shaped_dem, sun_direction, sun_targets, viewshed_targets, whitebox_observer,
                                      whitebox_reference, whitebox_scene_kwargs)

pytestmark = pytest.mark.gpu


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or scenes.CAM), **opts, **kw)


def _city():
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    return dem, verts, tris, _kw(dem, mesh_vertices=verts, mesh_indices=tris)


def test_the_library_exports_the_raster():
    from forge3d_amd import _native
    from forge3d_amd.session import TerrainSession

    assert _native.lib().f3d_session_raster is not None and _native.lib().f3d_abi_version() == 6
    assert callable(TerrainSession.visibility) and callable(TerrainSession.viewshed)


# ---- 1. device against oracle -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wanted(shaped):  # noqa: F811
    """The oracle's answers for every shape (computed once, shared, never written): [shape][(mode, curved)] -> bool (3, rows, cols)."""
    out = {}
    for shape, scene in shaped.items():
        out[shape] = {}
        for curved in (False, True):
            out[shape][TOWARD, curved] = contract_bits(scene, TOWARD, viewshed_targets(scene)[0], curved, None, 0.5)
            out[shape][ALONG, curved] = contract_bits(scene, ALONG, sun_targets(), curved, None, 1e-3)
        for v in out[shape].values():
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_the_oracle_bit_for_bit(shaped, wanted, shape):  # noqa: F811
    import torch

    scene = shaped[shape]
    with _session(scene.dem, scene.kw) as s:
        for curved in (False, True):
            for toward, targets, lift in ((True, viewshed_targets(scene)[0], 0.5), (False, sun_targets(), 1e-3)):
                want = wanted[shape][TOWARD if toward else ALONG, curved]
                masks, count = s.visibility(targets, toward=toward, curved=curved, lift=lift, count=True)
                assert masks.dtype == bool and masks.shape == want.shape and count.dtype == np.uint32
                wrong = int((masks != want).sum())
                assert wrong == 0, f"host form, toward={toward} curved={curved}: {wrong} of {want.size} bits differ from the oracle"
                assert np.array_equal(count, want.sum(0).astype(np.uint32))
                for k in (1, 2):
                    assert np.array_equal(s.visibility(targets[:k], toward=toward, curved=curved, lift=lift), want[:k]), f"K = {k}"
                assert np.array_equal(s.visibility(targets, toward=toward, curved=curved, lift=lift, masks=False, count=True), want.sum(0))
                d = torch.from_numpy(np.ascontiguousarray(targets)).cuda()
                dm, dc = s.visibility(d, toward=toward, curved=curved, lift=lift, count=True)
                assert dm.is_cuda and dm.dtype == torch.bool and np.array_equal(dm.cpu().numpy(), want), "device form"
                assert np.array_equal(dc.cpu().numpy().view(np.uint32), want.sum(0).astype(np.uint32))
                later = s.visibility(d, toward=toward, curved=curved, lift=lift, wait=False)  # NO_WAIT: in flight on the null stream
                torch.cuda.current_stream().synchronize()
                assert np.array_equal(later.cpu().numpy(), want), "device form, no wait"


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65)])
def test_regions_are_windows_of_the_whole_raster(shaped, wanted, region):  # noqa: F811
    scene = shaped[(63, 65)]
    r0, c0, r, c = region
    with _session(scene.dem, scene.kw) as s:
        got = s.visibility(viewshed_targets(scene)[0], toward=True, curved=True, lift=0.5, region=region)
        assert np.array_equal(got, wanted[(63, 65)][TOWARD, True][:, r0:r0 + r, c0:c0 + c])
        got = s.visibility(sun_targets(), toward=False, curved=False, lift=1e-3, region=region, masks=False, count=True)
        assert np.array_equal(got, wanted[(63, 65)][ALONG, False][:, r0:r0 + r, c0:c0 + c].sum(0))


def test_nan_targets_in_the_tensor_form_answer_zero(shaped, wanted):  # noqa: F811
    import torch

    scene = shaped[(63, 65)]
    good = viewshed_targets(scene)[0]
    with _session(scene.dem, scene.kw) as s:
        for slot, value in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            bad = good[0].copy()
            bad[slot] = value
            targets = torch.from_numpy(np.stack([good[0], bad, good[1]])).cuda()
            masks, count = s.visibility(targets, toward=True, curved=True, lift=0.5, count=True)
            masks = masks.cpu().numpy()
            assert not masks[1].any() and np.array_equal(masks[[0, 2]], wanted[(63, 65)][TOWARD, True][:2])
            assert np.array_equal(count.cpu().numpy(), masks.sum(0))
        with pytest.raises(ValueError, match="non-finite"):
            s.visibility(np.stack([good[0], bad]), toward=True, lift=0.5)


# ---- 2. the mesh -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_builder", [0, 2, 3])
def test_city_masks_equal_occluded_of_the_same_rays(harness, mesh_builder):  # noqa: F811
    dem, _, _, kw = _city()
    host = HostScene(harness, dem, kw)  # (the constants of this scene: the same fill_uniforms)
    try:
        ox = float(host.origin[0])
        with _session(dem, kw, mesh_builder=mesh_builder) as s:
            answers = {}
            for terrain_only in (False, True):
                for toward, targets, lift, curved in ((True, np.array([[0.3 * ox, 16.0, 0.2 * ox, 0.0], [0.0, 30.0, 0.0, 40.0]], f32), 0.5, False),
                                                      (False, sun_targets(), 1e-3, True)):
                    want = contract_bits(host, TOWARD if toward else ALONG, targets, curved, None, lift,
                                         occluded=lambda rays: s.occluded(rays, curved=curved, terrain_only=terrain_only))
                    got = s.visibility(targets, toward=toward, curved=curved, terrain_only=terrain_only, lift=lift)
                    assert np.array_equal(got, want), f"terrain_only={terrain_only} toward={toward}"
                    assert got.any() and not got.all()
                    answers[terrain_only, toward] = got
            assert (answers[False, False] != answers[True, False]).any(), "the boxes cast shadows"
            assert not (answers[False, False] & ~answers[True, False]).any()
            assert np.array_equal(answers[True, False], contract_bits(host, ALONG, sun_targets(), True, None, 1e-3)), "terrain only: the oracle"
    finally:
        host.close()


# ---- 3. the raster follows the live scene --------------------------------------------------------------------------------------
def test_session_sun_follows_a_rearm(harness):  # noqa: F811
    dem, _, _, kw = _city()
    with _session(dem, kw) as s:
        before = s.shadow_mask()
        host = HostScene(harness, dem, kw)
        try:
            assert np.array_equal(before, s.shadow_mask(host.sun)), "SESSION_SUN is ALONG_DIRECTION fed the armed sun's direction"
            assert abs(float(host.sun[1]) - np.sin(np.radians(kw["sun_elevation_deg"]))) < 1e-6
        finally:
            host.close()
        s.rearm(sun_elevation_deg=8.0)
        after = s.shadow_mask()  # (nothing between the update and the raster)
        with _session(dem, dict(kw, sun_elevation_deg=8.0)) as fresh:
            assert np.array_equal(after, fresh.shadow_mask())
        assert (after != before).any() and after.sum() < before.sum()


def test_rasters_follow_reterrain_and_remesh_without_a_wait():
    dem, verts, _, kw = _city()
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(np.float32)
    result = dem.copy()
    result[20:36, 20:36] = patch
    shift = np.array([6.0, 2.0, -4.0], np.float32)
    ox = -0.5 * scenes.SPAN
    observer = (0.3 * ox, 16.0, 0.2 * ox)
    with _session(dem, kw) as s:
        lit0, seen0 = s.shadow_mask(), s.viewshed(observer)
        s.reterrain(patch, at=(20, 20))
        lit1, seen1 = s.shadow_mask(), s.viewshed(observer)
        s.remesh(verts + shift)
        lit2, hours2 = s.shadow_mask(), s.sun_hours(sun_targets()[:, :3])
    with _session(result, kw) as fresh:
        assert np.array_equal(lit1, fresh.shadow_mask()) and np.array_equal(seen1, fresh.viewshed(observer)), "after reterrain"
    with _session(result, dict(kw, mesh_vertices=verts + shift)) as fresh:
        assert np.array_equal(lit2, fresh.shadow_mask()) and np.array_equal(hours2, fresh.sun_hours(sun_targets()[:, :3])), "after remesh"
    assert (lit0 != lit1).any() and (seen0 != seen1).any() and (lit1 != lit2).any()
    assert hours2.dtype == np.uint32 and hours2.max() == 3 and hours2.min() == 0


def test_a_strip_session_answers_the_whole_dem(shaped, wanted):  # noqa: F811
    scene = shaped[(63, 65)]
    with _session(scene.dem, scene.kw, row_begin=16, row_end=40) as s:
        assert np.array_equal(s.visibility(sun_targets(), toward=False, curved=True, lift=1e-3), wanted[(63, 65)][ALONG, True])


# ---- 4. read-only; the wrapper's methods ------------------------------------------------------------------------------------------
def test_rasters_change_nothing_a_frame_reads():
    dem, _, _, kw = _city()
    ox = -0.5 * scenes.SPAN
    with _session(dem, kw) as s, _session(dem, kw) as plain:
        fp = s.fingerprint()
        s.shadow_mask(), s.viewshed((0.3 * ox, 16.0, 0.2 * ox)), s.sun_hours(sun_targets()[:, :3]), s.viewshed((0.3 * ox, 0.2 * ox), curved=True)
        assert s.fingerprint() == fp
        n = 4
        for f in range(n):
            s.enqueue_frames(f, 1, f + 1 == n)
            s.shadow_mask(region=(f, 2 * f, 33, 40))
            s.viewshed((0.3 * ox, 16.0, 0.2 * ox), curved=True)
            plain.enqueue_frames(f, 1, f + 1 == n)
        got, want = s.resolve(n), plain.resolve(n)
        for k in ("rgba", "albedo", "normal", "depth"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.window_stats() == plain.window_stats()


def test_viewshed_shadow_mask_and_sun_hours(harness):  # noqa: F811
    dem = scenes.golden_dem(4)
    kw = _kw(dem)
    host = HostScene(harness, dem, kw)
    try:
        ox = float(host.origin[0])
        with _session(dem, kw) as s:
            obs = np.array([[0.3 * ox, 16.0, 0.2 * ox], [-0.3 * ox, 19.0, 0.1 * ox]], f32)
            lift = f32(f32(0.25) + f32(1e-3))
            want = contract_bits(host, TOWARD, np.concatenate([obs, np.full((2, 1), 30.0, f32)], 1), True, None, lift)
            one = s.viewshed(obs[0], target_height=0.25, max_distance=30.0, curved=True)
            assert one.dtype == bool and one.shape == dem.shape and np.array_equal(one, want[0])
            both = s.viewshed(obs, target_height=0.25, max_distance=30.0, curved=True)
            assert both.dtype == np.uint32 and np.array_equal(both, want.sum(0)), "several observers: the cumulative viewshed"
            # (x, z): standing observer_height above ground()
            xz = obs[:1, [0, 2]]
            y = s.ground(xz)[0] + f32(1.7)
            assert np.array_equal(s.viewshed(xz[0]), s.viewshed((xz[0, 0], y, xz[0, 1])))
            assert not s.viewshed((10.0 * ox, 0.0)).any(), "no ground to stand on: nothing seen"
            # the sun: directions below the horizontal are dropped and light nothing
            d = np.concatenate([sun_targets()[:, :3], np.array([[0.5, -0.2, 0.5], [1.0, 0.0, 0.0]], f32)])
            want = contract_bits(host, ALONG, sun_targets(), True, None, 1e-3)
            assert np.array_equal(s.sun_hours(d), want.sum(0))
            assert np.array_equal(s.shadow_mask(d[1]), want[1]) and np.array_equal(s.shadow_mask(d[1], region=(3, 4, 20, 21)), want[1][3:23, 4:25])
            assert np.array_equal(s.shadow_mask(d[1], curved=False), contract_bits(host, ALONG, sun_targets()[1], False, None, 1e-3)[0])
    finally:
        host.close()


# ---- 5. memory ---------------------------------------------------------------------------------------------------------------
def test_the_host_scratch_only_grows_and_the_tensor_form_takes_nothing(shaped):  # noqa: F811
    import torch

    scene = shaped[(63, 65)]
    n, words = 63 * 65, (63 * 65 + 63) // 64
    targets = sun_targets()
    with _session(scene.dem, scene.kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        s.visibility(torch.from_numpy(targets).cuda(), toward=False, lift=1e-3, count=True)
        assert s.info()["gpu_resource_bytes"] == bytes0, "the device form takes nothing"
        s.visibility(targets, toward=False, lift=1e-3)
        grown = s.info()["gpu_resource_bytes"]
        assert grown == bytes0 + 3 * words * 8 + 3 * 16, "masks and targets"
        s.visibility(targets, toward=False, lift=1e-3), s.visibility(targets[:2], toward=False, lift=1e-3), s.shadow_mask()
        assert s.info()["gpu_resource_bytes"] == grown, "a repeated or smaller call reuses the scratch"
        s.visibility(targets, toward=False, lift=1e-3, count=True)
        assert s.info()["gpu_resource_bytes"] == bytes0 + 3 * words * 8 + 3 * 16 + 4 * n, "a larger call grows it, the old one goes back"


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def _raw(s, targets, mode=1, flags=0, region=(0, 0, 64, 64), lift=1e-3, struct_size=None, masks=True, count=False, reserved=0, k=None):
    from forge3d_amd import _native

    q = _native.RasterDesc()
    q.struct_size = C.sizeof(_native.RasterDesc) if struct_size is None else struct_size
    q.mode, q.flags, q.lift, q.reserved = mode, flags, lift, reserved
    q.row0, q.col0, q.rows, q.cols = region
    q.target_count = (0 if targets is None else len(targets)) if k is None else k
    q.targets = None if targets is None else targets.ctypes.data
    n = min(max(q.rows * q.cols, 1), 64 * 64)  # (a region the call refuses is refused before anything is written)
    m = np.zeros((max(q.target_count, 1), (n + 63) // 64), np.uint64)
    c = np.zeros(n, np.uint32)
    q.masks, q.count = (m.ctypes.data if masks else None), (c.ctypes.data if count else None)
    s._check(s._lib.f3d_session_raster(s._handle, C.byref(q), s._err, len(s._err)))
    return m, c


def test_refusals_leave_the_session_rendering_what_it_rendered():
    dem, _, _, kw = _city()
    kw = scenes.fixed_frames(kw, 4)
    targets = np.ascontiguousarray(sun_targets())
    scratch = 3 * (64 * 64 // 64) * 8 + 3 * 16 + 4 * 64 * 64  # masks, targets, count (more than a create's own transient peak)
    with _session(dem, kw) as probe:
        need = probe.info()["gpu_resource_bytes"] + scratch
        want = probe.render()
    with _session(dem, kw, memory_budget_bytes=need - 1) as s:
        fp = s.fingerprint()
        for match, call in (
                ("struct_size", lambda: _raw(s, targets, struct_size=16)),
                ("raster mode must be", lambda: _raw(s, targets, mode=2)),
                ("unknown raster flags", lambda: _raw(s, targets, flags=32)),
                ("reserved", lambda: _raw(s, targets, reserved=1)),
                ("outside the 64x64 DEM", lambda: _raw(s, targets, region=(0, 1, 64, 64))),
                ("outside the 64x64 DEM", lambda: _raw(s, targets, region=(64, 0, 1, 1))),
                ("outside the 64x64 DEM", lambda: _raw(s, targets, region=(1, 0, 0xFFFFFFFF, 1))),
                ("empty raster region", lambda: _raw(s, targets, region=(0, 0, 0, 64))),
                ("empty raster region", lambda: _raw(s, targets, region=(3, 3, 5, 0))),
                ("lift must be finite", lambda: _raw(s, targets, lift=float("nan"))),
                ("lift must be finite", lambda: _raw(s, targets, lift=float("inf"))),
                ("non-finite", lambda: _raw(s, np.array([[0, 1, 0, 0], [0, np.nan, 0, 0]], np.float32))),
                ("SESSION_SUN", lambda: _raw(s, targets, flags=16)),
                ("SESSION_SUN", lambda: _raw(s, None, flags=16, mode=0)),
                ("NO_WAIT", lambda: _raw(s, targets, flags=8)),
                ("both null", lambda: _raw(s, targets, masks=False)),
                ("null targets", lambda: _raw(s, None, k=2))):
            with pytest.raises(ValueError, match=match):
                call()
            # (what a frame launch reads is what it read: the render that follows this refusal is the render before it)
            assert s.fingerprint() == fp and s.info()["gpu_resource_bytes"] == need - scratch, f"after the refusal '{match}'"
        with pytest.raises(RuntimeError, match="memory budget"):
            s.visibility(targets, toward=False, lift=1e-3, count=True)
        assert s.info()["gpu_resource_bytes"] == need - scratch and s.fingerprint() == fp
        with pytest.raises(ValueError, match="outside the 64x64 DEM"):
            s.viewshed((1e6, 1e6), region=(0, 0, 65, 64))  # (an observer with no ground under it: the region is still checked)
        m, c = _raw(s, targets[:0], count=True)  # K = 0 without SESSION_SUN: a successful no-op
        assert not m.any() and not c.any()
        assert s.visibility(targets[:2], toward=False, lift=1e-3, count=True)[0].shape == (2, 64, 64), "one target fewer fits"
        _same(s.render(), {k: v for k, v in want.items() if k != "gpu_resource_bytes"}, "after the refusals")
    with _session(dem, kw, memory_budget_bytes=need) as s:
        assert s.visibility(targets, toward=False, lift=1e-3, count=True)[0].shape == (3, 64, 64), "the budget that fits"
        with pytest.raises(ValueError, match="toward=False"):
            s.visibility(None, toward=True)
        with pytest.raises(ValueError, match="wait=False"):
            s.visibility(targets, toward=False, wait=False)


# ---- 7. the reference's own curved-earth golden --------------------------------------------------------------------------------
def test_whitebox_curved_golden_on_the_device():
    reference = whitebox_reference()
    dem, kw = whitebox_scene_kwargs()
    with _session(dem, kw, cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)}) as s:
        ox, oz = -0.5 * 255.0 * np.float64(f32(434.8)), -0.5 * 255.0 * np.float64(f32(431.9))
        obs = whitebox_observer((f32(ox), f32(oz)), (f32(434.8), f32(431.9)))[0, :3]
        curved = s.viewshed(obs, curved=True)
        flat = s.viewshed(obs)
        print(f"whitebox golden on the device: curved IoU {iou(curved, reference):.5f} ({int(curved.sum())} visible, "
              f"{int((curved ^ reference).sum())} flipped), flat control {iou(flat, reference):.7f}")
        assert iou(curved, reference) >= 0.98
        assert iou(flat, reference) < 0.98
