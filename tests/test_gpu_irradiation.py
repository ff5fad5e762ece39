"""Irradiation rasters on a live terrain session (f3d_session_irradiation; TerrainSession.irradiation / surface_normals /
insolation) on the device.

* the device against the host build of the same lane body (tests/irradiation_host), bit for bit -- energy, count, normals -- on
  the CPU suite's shapes (5x3, 33x33, 64x64, 65x63): host form, device-tensor form, NO_WAIT, curved and flat, HORIZONTAL and not,
  regions; NaN directions in the tensor form answer 0;
* the box city, with and without terrain_only: energy is the NumPy sequential sum of wt c over the pairs whose bit
  session.visibility() sets and whose c > 0, wt > 0, bit for bit, and count their number -- no oracle in it;
* after rearm / reterrain / remesh, with no host wait in between, a fresh session's; a strip session answers the whole DEM;
  fingerprint() and a render with irradiation calls interleaved are unchanged;
* the host scratch only grows; a call past memory_budget_bytes is refused and the session still renders; every refusal
  carries its message and leaves the render as it was;
* insolation() over a sun_track of one civil day is irradiation() plus sky_view_factor() as documented.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_gpu_reaim import H, W, _same
from test_session_irradiation_host import (CURVED, HORIZONTAL, TERRAIN_ONLY, Scene, contract_irradiation, contract_normals, contract_slope,  # noqa: F401
                                           directions, f32, irradiation_harness, irradiation_scenes, same_bits)
from test_session_raster_host import SHAPES, _kw

pytestmark = pytest.mark.gpu


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or scenes.CAM), **opts, **kw)


def _city():
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    return dem, verts, tris, _kw(dem, mesh_vertices=verts, mesh_indices=tris)


def _equal(got, want):
    """(energy, count) of the wrapper against a harness / contract answer."""
    energy, count = (np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in got)
    return same_bits(energy, want["energy"]) and np.array_equal(count.view(np.uint32), want["count"])


def test_the_library_exports_the_irradiation():
    from forge3d_amd import _native
    from forge3d_amd.session import TerrainSession

    assert _native.lib().f3d_session_irradiation is not None and _native.lib().f3d_abi_version() == 6
    assert callable(TerrainSession.irradiation) and callable(TerrainSession.surface_normals) and callable(TerrainSession.insolation)


# ---- 1. device against the host build of the lane body ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_the_host_body_bit_for_bit(irradiation_scenes, shape):  # noqa: F811
    import torch

    scene = irradiation_scenes[shape]
    terms = directions()
    with _session(scene.dem, scene.kw) as s:
        normals = s.surface_normals()
        assert normals.dtype == f32 and normals.shape == (*shape, 3)
        for curved in (False, True):
            for horizontal in (False, True):
                want = scene.irradiation(terms, (CURVED if curved else 0) | (HORIZONTAL if horizontal else 0))
                how = dict(curved=curved, horizontal=horizontal)
                got = s.irradiation(terms, count=True, **how)
                assert got[0].dtype == f32 and got[0].shape == shape and got[1].dtype == np.uint32 and got[1].shape == shape
                assert _equal(got, want), f"host form, {how}"
                assert same_bits(s.irradiation(terms[:, :3], terms[:, 3], **how), want["energy"]), "(K, 3) with weights"
                d = torch.from_numpy(terms).cuda()
                got = s.irradiation(d, count=True, **how)
                assert got[0].is_cuda and got[0].dtype == torch.float32 and got[1].dtype == torch.int32
                assert _equal(got, want), f"device form, {how}"
                later = s.irradiation(d, count=True, wait=False, **how)  # NO_WAIT: in flight on the null stream
                torch.cuda.current_stream().synchronize()
                assert _equal(later, want), f"device form, no wait, {how}"
                if not horizontal:
                    assert same_bits(normals, want["normal"]), "the normals the irradiation uses"
        for k in (1, 3):
            assert _equal(s.irradiation(terms[:k], count=True), scene.irradiation(terms[:k], CURVED)), f"K = {k}"
        later = s.surface_normals(wait=False)
        torch.cuda.current_stream().synchronize()
        assert later.is_cuda and same_bits(later.cpu().numpy(), normals)


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65)])
def test_regions_are_windows_of_the_whole_raster(irradiation_scenes, region):  # noqa: F811
    scene = irradiation_scenes[(63, 65)]
    want = scene.irradiation(directions(), CURVED)
    r0, c0, r, c = region
    with _session(scene.dem, scene.kw) as s:
        energy, count = s.irradiation(directions(), region=region, count=True)
        assert same_bits(energy, want["energy"][r0:r0 + r, c0:c0 + c]) and np.array_equal(count, want["count"][r0:r0 + r, c0:c0 + c])
        assert same_bits(s.surface_normals(region), want["normal"][r0:r0 + r, c0:c0 + c])


def test_nan_directions_in_the_tensor_form_answer_zero(irradiation_scenes):  # noqa: F811
    import torch

    from forge3d_amd import _native

    scene = irradiation_scenes[(63, 65)]
    good = directions(3)
    want = scene.irradiation(good, CURVED)
    with _session(scene.dem, scene.kw) as s:
        for bad in ([np.nan, 0.5, 0.2, 9.0], [0.3, 0.5, np.inf, 9.0], [0.3, 0.5, 0.2, np.nan], [0.3, 0.5, 0.2, -4.0], [0.0, 0.0, 0.0, 9.0]):
            terms = np.concatenate([good[:2], np.array([bad], f32), good[2:]])
            assert _equal(s.irradiation(torch.from_numpy(terms).cuda(), count=True), want), bad
            # (the wrapper gives y <= 0 and NaN y weight 0 before the call: here the lanes see the term as it is)
            q = _native.IrradiationDesc()
            q.struct_size = C.sizeof(_native.IrradiationDesc)
            q.flags = _native.IRRADIATION_CURVED | _native.IRRADIATION_DEVICE_POINTERS
            q.rows, q.cols, q.lift, q.direction_count = 63, 65, 1e-3, 4
            d = torch.from_numpy(terms).cuda()
            energy, count = torch.empty(63 * 65, dtype=torch.float32, device="cuda"), torch.empty(63 * 65, dtype=torch.int32, device="cuda")
            q.directions, q.energy, q.count = d.data_ptr(), energy.data_ptr(), count.data_ptr()
            s._check(s._lib.f3d_session_irradiation(s._handle, C.byref(q), s._err, len(s._err)))
            assert _equal((energy.reshape(63, 65), count.reshape(63, 65)), want), f"raw device form, {bad}"
        with pytest.raises(ValueError, match="non-finite"):
            s.irradiation(np.concatenate([good, np.array([[np.nan, 0.5, 0.2, 9.0]], f32)]))


# ---- 2. composition: the rasters that are already tested, no oracle -------------------------------------------------------------
@pytest.mark.parametrize("terrain_only", [False, True], ids=["mesh", "terrain_only"])
def test_city_energy_is_the_sum_over_the_pairs_visibility_lights(irradiation_harness, terrain_only):  # noqa: F811
    dem, _, _, kw = _city()
    host = Scene(irradiation_harness, dem, kw)  # (the constants of this scene: origin, spacing)
    terms = directions()
    try:
        with _session(dem, kw) as s:
            for curved in (False, True):
                bits = s.visibility(terms[:, :3], toward=False, curved=curved, terrain_only=terrain_only, lift=s.SURFACE_BIAS)
                want = contract_irradiation(host, terms, curved, bits=bits)
                got = s.irradiation(terms, curved=curved, terrain_only=terrain_only, count=True)
                assert _equal(got, want), f"curved={curved}"
                assert np.array_equal(got[1], (want["go"] & bits).sum(0)), "count: the number of such pairs"
                assert (want["go"] & ~bits).any() and (want["go"] & bits).any() and (~want["go"]).any()
            assert same_bits(s.surface_normals(), want["normal"])
    finally:
        host.close()


def test_the_boxes_only_ever_shade():
    dem, _, _, kw = _city()
    with _session(dem, kw) as s:
        full, bare = s.irradiation(directions(), count=True), s.irradiation(directions(), terrain_only=True, count=True)
        assert (full[1] <= bare[1]).all() and (full[1] < bare[1]).any() and (full[0] <= bare[0]).all()


# ---- 3. the raster follows the live scene ----------------------------------------------------------------------------------------
def test_irradiation_follows_rearm_reterrain_and_remesh_without_a_wait():
    dem, verts, _, kw = _city()
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(np.float32)
    result = dem.copy()
    result[20:36, 20:36] = patch
    shift = np.array([6.0, 2.0, -4.0], np.float32)
    terms = directions()
    with _session(dem, kw) as s:
        e0 = s.irradiation(terms, count=True)
        s.rearm(sun_elevation_deg=8.0)
        e1 = s.irradiation(terms, count=True)  # (nothing between the update and the raster)
        s.reterrain(patch, at=(20, 20))
        e2, n2 = s.irradiation(terms, count=True), s.surface_normals()
        s.remesh(verts + shift)
        e3 = s.irradiation(terms, count=True)
    assert same_bits(e0[0], e1[0]) and np.array_equal(e0[1], e1[1]), "the directions are the call's: a rearm changes nothing"
    with _session(result, kw) as fresh:
        got = fresh.irradiation(terms, count=True)
        assert same_bits(e2[0], got[0]) and np.array_equal(e2[1], got[1]) and same_bits(n2, fresh.surface_normals()), "after reterrain"
    with _session(result, dict(kw, mesh_vertices=verts + shift)) as fresh:
        got = fresh.irradiation(terms, count=True)
        assert same_bits(e3[0], got[0]) and np.array_equal(e3[1], got[1]), "after remesh"
    assert (e1[0] != e2[0]).any() and (e2[1] != e3[1]).any()


def test_a_strip_session_answers_the_whole_dem(irradiation_scenes):  # noqa: F811
    scene = irradiation_scenes[(63, 65)]
    want = scene.irradiation(directions(), CURVED)
    with _session(scene.dem, scene.kw, row_begin=16, row_end=40) as s:
        assert _equal(s.irradiation(directions(), count=True), want) and same_bits(s.surface_normals(), want["normal"])


def test_irradiation_changes_nothing_a_frame_reads():
    dem, _, _, kw = _city()
    terms = directions()
    with _session(dem, kw) as s, _session(dem, kw) as plain:
        fp = s.fingerprint()
        s.irradiation(terms), s.irradiation(terms[:3], horizontal=True, region=(3, 4, 20, 21), count=True), s.surface_normals()
        assert s.fingerprint() == fp
        n = 4
        for f in range(n):
            s.enqueue_frames(f, 1, f + 1 == n)
            s.irradiation(terms, region=(f, 2 * f, 33, 40))
            s.surface_normals()
            plain.enqueue_frames(f, 1, f + 1 == n)
        got, want = s.resolve(n), plain.resolve(n)
        for k in ("rgba", "albedo", "normal", "depth"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.window_stats() == plain.window_stats()


# ---- 4. memory -------------------------------------------------------------------------------------------------------------------
def test_the_host_scratch_only_grows_and_the_tensor_form_takes_nothing(irradiation_scenes):  # noqa: F811
    import torch

    scene = irradiation_scenes[(63, 65)]
    n = 63 * 65
    room = lambda b: (b + 15) & ~15
    terms = directions()
    with _session(scene.dem, scene.kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        s.irradiation(torch.from_numpy(terms).cuda(), count=True), s.surface_normals(wait=False)
        torch.cuda.synchronize()
        assert s.info()["gpu_resource_bytes"] == bytes0, "the device form takes nothing"
        s.irradiation(terms[:3])
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(4 * n) + 3 * 16, "energy and the directions"
        s.irradiation(terms, count=True)
        grown = s.info()["gpu_resource_bytes"]
        assert grown == bytes0 + room(8 * n) + 8 * 16, "a larger call grows it, the old one goes back"
        s.irradiation(terms, count=True), s.irradiation(terms[:2]), s.shadow_mask(), s.sky_view_factor(4)
        assert s.info()["gpu_resource_bytes"] == grown, "a repeated or smaller call, another raster included, reuses the scratch"
        s.surface_normals()
        assert s.info()["gpu_resource_bytes"] == bytes0 + room(12 * n), "the normals alone: no directions"


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(s, terms, flags=0, region=(0, 0, 64, 64), lift=1e-3, struct_size=None, energy=True, count=False, normal=False, reserved=0, k=None):
    from forge3d_amd import _native

    q = _native.IrradiationDesc()
    q.struct_size = C.sizeof(_native.IrradiationDesc) if struct_size is None else struct_size
    q.flags, q.lift, q.reserved = flags, lift, reserved
    q.row0, q.col0, q.rows, q.cols = region
    q.direction_count = (0 if terms is None else len(terms)) if k is None else k
    q.directions = None if terms is None or len(terms) == 0 else terms.ctypes.data
    n = min(max(q.rows * q.cols, 1), 64 * 64)  # (a call that is refused is refused before anything is written)
    e, c, v = np.zeros(n, f32), np.zeros(n, np.uint32), np.zeros((n, 3), f32)
    q.energy, q.count, q.normal = (e.ctypes.data if energy else None), (c.ctypes.data if count else None), (v.ctypes.data if normal else None)
    s._check(s._lib.f3d_session_irradiation(s._handle, C.byref(q), s._err, len(s._err)))
    return e, c, v


def test_refusals_leave_the_session_rendering_what_it_rendered():
    dem, _, _, kw = _city()
    kw = scenes.fixed_frames(kw, 4)
    terms = np.ascontiguousarray(directions())
    scratch = (4 + 4 + 12) * 64 * 64 + 8 * 16  # energy, count, normals, directions (more than a create's own transient peak)
    with _session(dem, kw) as probe:
        need = probe.info()["gpu_resource_bytes"] + scratch
        want = probe.render()
    bad = lambda slot, value: np.concatenate([terms[:1], [[*terms[1, :slot], value, *terms[1, slot + 1:]]]]).astype(f32)
    with _session(dem, kw, memory_budget_bytes=need - 1) as s:
        fp = s.fingerprint()
        for match, call in (
                ("struct_size", lambda: _raw(s, terms, struct_size=16)),
                ("unknown irradiation flags", lambda: _raw(s, terms, flags=32)),
                ("unknown irradiation flags", lambda: _raw(s, terms, flags=1 << 31)),
                ("reserved", lambda: _raw(s, terms, reserved=1)),
                ("NO_WAIT needs DEVICE_POINTERS", lambda: _raw(s, terms, flags=8)),
                ("outside the 64x64 DEM", lambda: _raw(s, terms, region=(0, 1, 64, 64))),
                ("outside the 64x64 DEM", lambda: _raw(s, terms, region=(64, 0, 1, 1))),
                ("outside the 64x64 DEM", lambda: _raw(s, terms, region=(1, 0, 0xFFFFFFFF, 1))),
                ("empty irradiation region", lambda: _raw(s, terms, region=(0, 0, 0, 64))),
                ("empty irradiation region", lambda: _raw(s, terms, region=(3, 3, 5, 0))),
                ("lift must be finite", lambda: _raw(s, terms, lift=float("nan"))),
                ("lift must be finite", lambda: _raw(s, terms, lift=float("inf"))),
                ("all null", lambda: _raw(s, terms, energy=False)),
                ("need direction_count > 0", lambda: _raw(s, terms[:0])),
                ("need direction_count > 0", lambda: _raw(s, terms[:0], energy=False, count=True, normal=True)),
                ("null directions", lambda: _raw(s, None, k=2)),
                ("direction 1 has a non-finite component", lambda: _raw(s, bad(0, np.nan))),
                ("direction 1 has a non-finite component", lambda: _raw(s, bad(1, np.inf))),
                ("direction 1 has a non-finite component", lambda: _raw(s, bad(3, np.nan))),
                ("direction 1 has a negative weight", lambda: _raw(s, bad(3, -1.0)))):
            with pytest.raises(ValueError, match=match):
                call()
            # (what a frame launch reads is what it read: the render that follows this refusal is the render before it)
            assert s.fingerprint() == fp and s.info()["gpu_resource_bytes"] == need - scratch, f"after the refusal '{match}'"
        with pytest.raises(RuntimeError, match="memory budget"):
            _raw(s, terms, count=True, normal=True)
        assert s.info()["gpu_resource_bytes"] == need - scratch and s.fingerprint() == fp
        assert s.irradiation(terms, count=True)[0].shape == (64, 64), "without the normals it fits"
        _same(s.render(), {k: v for k, v in want.items() if k != "gpu_resource_bytes"}, "after the refusals")
    with _session(dem, kw, memory_budget_bytes=need) as s:
        e, c, v = _raw(s, terms, count=True, normal=True)  # the budget that fits
        assert (e > 0).any() and (c > 0).any() and np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max() < 4e-7
        assert same_bits(_raw(s, terms[:0], energy=False, normal=True)[2], v), "K = 0 with the normals alone"
        with pytest.raises(ValueError, match="wait=False"):
            s.irradiation(terms, wait=False)
        with pytest.raises(ValueError, match="must not be negative"):
            s.irradiation(terms, region=(0, -1, 4, 4))


# ---- 6. insolation ---------------------------------------------------------------------------------------------------------------
def test_insolation_is_irradiation_plus_the_sky_view_term(irradiation_scenes):  # noqa: F811
    from forge3d_amd import insolation

    scene = irradiation_scenes[(33, 33)]
    track = insolation.sun_track((2024, 3, 20), 46.85, -121.76, tz_offset_hours=-8.0)
    assert 20 <= len(track["utc"]) <= 26
    dni, dhi = insolation.clear_sky(track["elevation_deg"])
    with _session(scene.dem, scene.kw) as s:
        out = s.insolation(track)
        assert set(out) == {"direct", "diffuse", "global"} and all(v.dtype == f32 and v.shape == (33, 33) for v in out.values())
        weights = (dni * track["hours"]).astype(f32)
        assert same_bits(out["direct"], s.irradiation(track["directions"], weights))
        assert same_bits(out["direct"], scene.irradiation(s.irradiation_terms(track["directions"], weights), CURVED)["energy"])
        assert same_bits(out["diffuse"], s.sky_view_factor(16) * f32((dhi * track["hours"]).sum()))
        assert same_bits(out["global"], out["direct"] + out["diffuse"]) and out["direct"].max() > 1000.0 and out["diffuse"].min() > 0.0
        flat = s.insolation(track, dni=np.full(len(dni), 500.0), dhi=np.zeros(len(dni)), horizontal=True, region=(2, 3, 8, 9), azimuths=8)
        assert same_bits(flat["direct"], s.irradiation(track["directions"], (500.0 * track["hours"]).astype(f32), horizontal=True, region=(2, 3, 8, 9)))
        assert not flat["diffuse"].any() and same_bits(flat["global"], flat["direct"])
        with pytest.raises(TypeError):
            s.insolation(track, wait=False)
