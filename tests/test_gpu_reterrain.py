"""`-m gpu`: re-terrain of a live terrain session (f3d_session_reterrain: a re-aim under new DEM samples), byte for byte
against fresh renders.

A re-terrained session must render exactly what a new session (or the one-shot call, or the CPU oracle) renders on the
resulting DEM: all four outputs, frames, variance, converged, the certificates and EVERY fingerprint entry -- leaf table,
band tables and terrain scalars included -- after each edit.  A chain of edits on the 64x64 golden DEM -- a bump, a pit, one
corner sample, the last row, one column (patches), the DEM turned round, another exaggeration, the original again (whole
DEMs), a patch together with a new camera, sun and seed -- over the session forms (fused frames, frames in flight, bands on
several streams, 1 / 4 / 8 sample lanes), with a mesh (re-meshed and re-terrained in turn), the AETHER post, curvature on a
small sphere, two row strips, and under every poison pattern of the allocator (in child processes); a 2049^2 DEM once; two
sessions on one cached DEM; the memory it must not take; refusals; a re-terrain enqueued behind frames and a resolve
without a host wait and after a pool trim; render_terrain_dem_sequence.

Every edit is in the picture: the share of pixels whose depth differs from the unedited render, for the edit alone, has a
floor at roughly 0.6 to 0.7 of what the CPU oracle gives on this scene (bump 0.0161, pit 0.0252, corner 0.0011, edge
0.0869, col 0.0221, full 0.554, exag 0.579).
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import scenes
from test_gpu_reaim import AOVS, CHAIN, H, ORBIT, SCALARS, W, _golden, _session, _state

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EDITS = ("bump", "pit", "corner", "edge", "col", "full", "exag", "back", "combined")
FLOORS = {"bump": 0.010, "pit": 0.015, "corner": 3.0 / (W * H), "edge": 0.05, "col": 0.015, "full": 0.40, "exag": 0.40}
CAM_7 = CHAIN[3][0]


def _steps(dem, exaggeration):
    """The chain on `dem`: dicts with the call (heightmap, at, exaggeration, camera, change), the DEM and exaggeration the
    session holds afterwards (`dem`, `exag`), and the edit alone on the original DEM (`alone`, `alone_exag`)."""
    d = dem.copy()
    ex = exaggeration
    out = []

    def patch(name, rows, cols, values, camera=None, change=None):
        nonlocal d
        d = d.copy()
        d[rows, cols] = values
        alone = dem.copy()
        alone[rows, cols] = values
        block = np.ascontiguousarray(d[rows, cols])
        out.append(dict(name=name, heightmap=block, at=(rows.start, cols.start), exaggeration=None, camera=camera, change=change or {},
                        dem=d, exag=ex, alone=alone, alone_exag=exaggeration))

    y, x = np.mgrid[0:12, 0:12]
    patch("bump", slice(26, 38), slice(26, 38), dem[26:38, 26:38] + (0.35 * np.exp(-((y - 5.5) ** 2 + (x - 5.5) ** 2) / 18.0)).astype(np.float32))
    patch("pit", slice(40, 49), slice(10, 27), np.float32(0.0))
    patch("corner", slice(0, 1), slice(0, 1), np.float32(1.0))
    patch("edge", slice(63, 64), slice(0, 64), dem[63:64, :] + np.float32(0.2))
    patch("col", slice(0, 64), slice(31, 32), dem[:, 31:32] + np.float32(0.15))
    d = np.ascontiguousarray(d[::-1, ::-1])
    out.append(dict(name="full", heightmap=d, at=None, exaggeration=None, camera=None, change={}, dem=d, exag=ex,
                    alone=np.ascontiguousarray(dem[::-1, ::-1]), alone_exag=exaggeration))
    ex = float(np.float32(1.5 * exaggeration))
    out.append(dict(name="exag", heightmap=d, at=None, exaggeration=ex, camera=None, change={}, dem=d, exag=ex, alone=dem, alone_exag=ex))
    d, ex = dem.copy(), exaggeration
    out.append(dict(name="back", heightmap=d, at=None, exaggeration=ex, camera=None, change={}, dem=d, exag=ex, alone=None, alone_exag=None))
    patch("combined", slice(8, 20), slice(38, 52), dem[8:20, 38:52] + np.float32(0.3), CAM_7,
          dict(sun_azimuth_deg=80.0, sun_elevation_deg=20.0, seed=11, max_frames=3, min_frames=3))
    assert tuple(s["name"] for s in out) == EDITS
    return out


def _held(cam, kw, steps):
    """(DEM, camera, render keywords) of every step: a re-terrain keeps the camera and every value it is not given."""
    held, camera, out = dict(kw), dict(cam), []
    for st in steps:
        held = {**held, **st["change"], "exaggeration": st["exag"]}
        camera = dict(st["camera"]) if st["camera"] is not None else camera
        out.append((st["dem"], dict(camera), held))
    return out


def _apply(s, st):
    s.reterrain(st["heightmap"], st["camera"], at=st["at"], exaggeration=st["exaggeration"], **st["change"])


def _same(got, want, what=""):
    """Bit for bit on the outputs and on every scalar but gpu_resource_bytes (the staging buffer: checked apart)."""
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key}"
    for key in SCALARS:
        if key in want and key != "gpu_resource_bytes":
            assert got[key] == want[key], f"{what}: {key} {got[key]!r} != {want[key]!r}"


def _differs(a, b):
    return float(((a != b) & ~(np.isnan(a) & np.isnan(b))).mean())


def _chain(dem, cam, kw, oneshot=False, with_oracle=False, before_step=None, **opts):
    """Re-terrain one session along the chain; every step against a fresh session on the resulting DEM (and the one-shot,
    and the oracle); returns the results."""
    import forge3d_amd as f3d

    steps = _steps(dem, kw["exaggeration"])
    s = _session(dem, cam, kw, **opts)
    out = []
    try:
        previous = None
        for i, (st, (d, c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            name = st["name"]
            if before_step is not None:
                k = before_step(s, i, k)
            _apply(s, st)
            with _session(d, c, k, **opts) as fresh:
                got_state, want_state = _state(s), _state(fresh)
                assert got_state[1] == want_state[1], f"step {i} ({name}): certificates"
                differ = sorted(key for key in want_state[0] if got_state[0][key] != want_state[0][key])
                assert not differ, f"step {i} ({name}): fingerprint entries {differ} differ"
                want = fresh.render()
            got = s.render()
            _same(got, want, f"step {i} ({name}) vs a fresh session")
            assert got["gpu_resource_bytes"] >= want["gpu_resource_bytes"], (i, name)
            if previous is not None:  # (so that the comparison above means something: the edit changed the picture)
                assert not np.array_equal(got["depth"], previous["depth"], equal_nan=True), f"step {i} ({name}) renders the step before"
            previous = got
            if oneshot:
                _same(got, f3d.hybrid_render_terrain_reference(d, W, H, c, **k), f"step {i} ({name}) vs the one-shot")
            if with_oracle:
                from oracle import oracle

                want = oracle.render(d, W, H, c, **k)
                for key in AOVS:
                    assert np.array_equal(got[key], want[key], equal_nan=True), (i, name, key, "oracle")
            out.append(got)
    finally:
        s.close()
    return out


def test_chain_on_the_golden_dem_equals_fresh_sessions_one_shots_and_the_oracle():
    import forge3d_amd as f3d

    dem, cam, kw = _golden()
    assert dem.shape == (64, 64)
    _chain(dem, cam, kw, oneshot=True, with_oracle=True)
    # every edit, alone on the original DEM, is in the picture (floors from the CPU oracle: the module's docstring)
    unedited = f3d.hybrid_render_terrain_reference(dem, W, H, cam, **kw)["depth"]
    for st in _steps(dem, kw["exaggeration"]):
        if st["name"] not in FLOORS:
            continue
        alone = f3d.hybrid_render_terrain_reference(st["alone"], W, H, cam, **dict(kw, exaggeration=st["alone_exag"]))["depth"]
        share = _differs(alone, unedited)
        print(f"{st['name']}: depth differs from the unedited render on {share:.4f} of the pixels (floor {FLOORS[st['name']]:.4f})")
        assert share >= FLOORS[st["name"]], (st["name"], share)


@pytest.mark.parametrize("opts", [dict(frames_in_flight=0), dict(frames_in_flight=4), dict(frames_in_flight=0, bands=3, band_streams=2)],
                         ids=["fused", "in-flight-4", "bands"])
def test_chain_across_session_forms(opts):
    dem, cam, kw = _golden()
    _chain(dem, cam, kw, **opts)


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_chain_across_sample_lanes(lanes):
    from forge3d_amd.session import kernel_variant

    dem, cam, kw = _golden()
    _chain(dem, cam, dict(kw, spp=8), frames_in_flight=0, kernel_variant=kernel_variant(sample_lanes=lanes))


def test_chain_on_a_mesh_scene_remeshed_and_reterrained_in_turn():
    dem, cam, kw = _golden()
    v, t = scenes.box_city(n_boxes=30, seed=5)
    kw = dict(kw, mesh_vertices=v, mesh_indices=t)

    def remesh_first(s, i, k):  # before every re-terrain the mesh moves too (a refit of the session's own tree)
        moved = (v + np.float32([0.7 * (i + 1), 0.2 * i, -0.5 * (i + 1)])).astype(np.float32)
        s.remesh(moved)
        return dict(k, mesh_vertices=moved)

    steps = _steps(dem, kw["exaggeration"])
    s = _session(dem, cam, kw)
    try:
        for i, (st, (d, c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            k = remesh_first(s, i, k)
            _apply(s, st)
            with _session(d, c, k) as fresh:
                got_state, want_state = _state(s), _state(fresh)
                assert got_state[1] == want_state[1], f"step {i} ({st['name']}): certificates"
                tree = ("mesh_scalars", "bvh_nodes", "bvh_triangles")  # (a refitted tree is not a fresh one: tests/test_gpu_remesh.py)
                differ = sorted(key for key in want_state[0] if got_state[0][key] != want_state[0][key] and key not in tree)
                assert not differ, f"step {i} ({st['name']}): fingerprint entries {differ} differ"
                _same(s.render(), fresh.render(), f"mesh scene step {i} ({st['name']})")
    finally:
        s.close()


def test_chain_with_the_aether_post():
    import forge3d_amd as f3d
    from forge3d_amd import _native

    dem, cam, kw = _golden()
    handle = _native._resolve_atmosphere({"turbidity": 3.0})
    steps = _steps(dem, kw["exaggeration"])
    s = _session(dem, cam, dict(kw, atmosphere=handle))
    try:
        for i, (st, (d, c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            _apply(s, st)
            got = s.render()
            _same(got, f3d.hybrid_render_terrain_reference(d, W, H, c, atmosphere={"turbidity": 3.0}, **k), f"aether step {i} ({st['name']})")
    finally:
        s.close()
    assert not np.array_equal(got["rgba"], f3d.hybrid_render_terrain_reference(d, W, H, c, **k)["rgba"])  # (the post is on)


def test_chain_on_the_small_sphere_curvature_scene():
    dem, cam, kw = _golden()
    span = kw["spacing"][0] * max(dem.shape)
    _chain(dem, cam, dict(kw, earth_model="sphere", refraction_model="none", sphere_radius_m=3.0 * span), oneshot=True)


@pytest.mark.parametrize("in_flight", [0, 4])
def test_reterrained_row_strips_equal_the_whole_image(in_flight):
    """Two strips with caller-owned reservoirs and the device-copy halo exchange (as test_gpu_reaim's strip test)."""
    import torch

    import forge3d_amd as f3d
    from forge3d_amd.session import HALO_ROWS as R, TerrainSession, reservoir_buffer_bytes

    dem, cam, kw = _golden()
    bounds = [(0, 29), (29, 64)]
    dev = torch.device("cuda", 0)
    bufs = [[torch.zeros(reservoir_buffer_bytes(e - b, W), dtype=torch.uint8, device=dev) for _ in range(2)] for b, e in bounds]
    sessions = [TerrainSession(dem, W, H, cam, row_begin=b, row_end=e, frames_in_flight=in_flight,
                               ext_reservoirs=(res[0].data_ptr(), res[1].data_ptr()), **kw) for (b, e), res in zip(bounds, bufs)]
    row = W * 16

    def exchange(which):
        torch.cuda.synchronize()
        up, dn = bufs[0][which], bufs[1][which]
        rows_up = bounds[0][1] - bounds[0][0]
        dn[0:R * row] = up[rows_up * row:(rows_up + R) * row]
        up[(rows_up + R) * row:(rows_up + 2 * R) * row] = dn[R * row:2 * R * row]
        torch.cuda.synchronize()

    def render(frames):
        f = 0
        while f < frames:
            if in_flight:
                n = sessions[0].trace_batch(f, frames - f)
                for s in sessions:
                    s.enqueue_trace(f, n)
                for g in range(f, f + n):
                    for s in sessions:
                        s.enqueue_merge(g)
                    exchange(g & 1)
                f += n
            else:
                for s in sessions:
                    s.enqueue_frames(f, 1, False)
                exchange(f & 1)
                f += 1
        parts = [s.resolve(frames) for s in sessions]
        return {key: np.concatenate([p[key] for p in parts], axis=0) for key in AOVS}

    steps = _steps(dem, kw["exaggeration"])
    try:
        render(4)
        for i, (st, (d, c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            for s in sessions:
                _apply(s, st)
            got = render(int(k["max_frames"]))
            want = f3d.hybrid_render_terrain_reference(d, W, H, c, **k)
            for key in AOVS:
                assert np.array_equal(got[key], want[key], equal_nan=True), (i, st["name"], key)
    finally:
        for s in sessions:
            s.close()


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_reterrain as t
dem, cam, kw = t._golden()
out = {}
for name, opts in (("auto", {}), ("fused", {"frames_in_flight": 0})):
    s = t._session(dem, cam, kw, **opts)
    for j, st in enumerate(t._steps(dem, kw["exaggeration"])):
        t._apply(s, st)
        r = s.render()
        for key in t.AOVS:
            out[f"{name}_{j}_{key}"] = r[key]
    s.close()
np.savez(sys.argv[2], **out)
"""


def _chains_in_children(paths):
    """One child per (poison pattern or None, path), side by side (four processes: their start-up is most of their time)."""
    procs = []
    for poison, path in paths:
        env = dict(os.environ)
        env.pop("F3D_POISON", None)
        if poison is not None:
            env["F3D_POISON"] = str(poison)
        procs.append(subprocess.Popen([sys.executable, "-c", _CHILD, str(ROOT), str(path)], env=env, stdout=subprocess.DEVNULL,
                                      stderr=subprocess.PIPE, text=True))
    ends = [(p.communicate(timeout=300)[1], p.returncode) for p in procs]
    for (poison, _), (stderr, code) in zip(paths, ends):
        assert code == 0, (poison, stderr[-3000:])
    return [dict(np.load(path)) for _, path in paths]


def test_the_chain_under_every_poison_pattern_equals_the_plain_run():
    """What the table passes read they or the device copies must have written: with the allocator filling the session's own
    tables and its staging buffer with a pattern, a record or a sample the passes forget would carry it into the march."""
    with tempfile.TemporaryDirectory() as tmp:
        patterns = (0, 0x5A, 0xFF)
        plain, *poisoned = _chains_in_children([(None, Path(tmp) / "plain.npz")] + [(p, Path(tmp) / f"p{p}.npz") for p in patterns])
        assert len(plain) == 2 * len(EDITS) * len(AOVS)
        for pattern, got in zip(patterns, poisoned):
            assert sorted(got) == sorted(plain)
            for key in plain:
                assert np.array_equal(got[key], plain[key], equal_nan=True), (pattern, key)


def test_a_2049_dem_whole_and_a_300_patch_equal_fresh_sessions():
    """Twelve levels: the tile pass over 1 024 workgroups and the top pass through global memory.  Run once."""
    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem = datasets.rainier_proxy(2049)
    assert dem.shape == (2049, 2049)
    spacing = 10.0
    cam = {"origin": (2500.0, float(dem.max()) + 2500.0, 6500.0), "look_at": (0.0, float(dem.mean()), 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 50.0,
           "exposure": 1.0}
    kw = dict(spacing=(spacing, spacing), exaggeration=1.0, albedo=(0.6, 0.6, 0.6), sun_azimuth_deg=302.0, sun_elevation_deg=24.0, spp=2,
              max_frames=2, min_frames=2, variance_threshold=1e30)
    whole = np.ascontiguousarray(dem[::-1, :] * np.float32(0.8))
    patched = whole.copy()
    yy, xx = np.mgrid[0:300, 0:300]
    relief = float(dem.max() - dem.min())
    patched[870:1170, 1000:1300] += (0.5 * relief * np.exp(-((yy - 150.0) ** 2 + (xx - 150.0) ** 2) / 8000.0)).astype(np.float32)
    with TerrainSession(dem, 64, 64, cam, **kw) as s:
        before = s.render()
        for name, d, call in (("whole", whole, lambda: s.reterrain(whole)), ("patch", patched, lambda: s.reterrain(patched[870:1170, 1000:1300], at=(870, 1000)))):
            call()
            with TerrainSession(d, 64, 64, cam, **kw) as fresh:
                got_state, want_state = _state(s), _state(fresh)
                differ = sorted(key for key in want_state[0] if got_state[0][key] != want_state[0][key])
                assert not differ and got_state[1] == want_state[1], (name, differ)
                want = fresh.render()
            got = s.render()
            _same(got, want, f"2049^2 {name}")
            assert not np.array_equal(got["depth"], before["depth"], equal_nan=True), name
            before = got


def test_a_reterrain_leaves_the_cached_dem_of_other_sessions_alone():
    dem, cam, kw = _golden()
    st = _steps(dem, kw["exaggeration"])[0]
    with _session(dem, cam, kw) as a, _session(dem, cam, kw) as b:
        before = _state(b)
        assert _state(a) == before  # one cached DEM, two sessions
        original = b.render()
        _apply(a, st)
        got = a.render()
        assert not np.array_equal(got["depth"], original["depth"], equal_nan=True)
        b.rearm()
        assert _state(b) == before
        _same(b.render(), original, "the session that shares the DEM")
        from forge3d_amd import _native

        entries = _native.lib().f3d_scene_cache_entries()
        with _session(dem, cam, kw) as c:  # (the cache entry itself still holds the original DEM: a hit, and the original picture)
            assert _native.lib().f3d_scene_cache_entries() == entries
            assert c.setup_ms()["upload"] == 0.0 and c.setup_ms()["tables"] == 0.0
            assert _state(c) == before
            _same(c.render(), original, "a session created afterwards with the original DEM")
        with _session(st["dem"], cam, kw) as fresh:
            _same(got, fresh.render(), "the re-terrained session")


def test_ten_reterrains_after_the_first_take_no_memory_and_the_smallest_budget_refuses_the_first():
    dem, cam, kw = _golden()
    steps = _steps(dem, kw["exaggeration"])
    opts = dict(frames_in_flight=0)
    with _session(dem, cam, kw, **opts) as s:
        need = s.info()["gpu_resource_bytes"]
        s.render()  # (the read-back of a picture sets peak_host_visible_bytes once; no device allocation)
        created = s.info()
        assert created["gpu_resource_bytes"] == need
        s.reterrain(dem * np.float32(0.9))  # (the whole DEM first: the largest block, the staging buffer never grows again)
        first = s.info()
        assert first["gpu_resource_bytes"] == created["gpu_resource_bytes"] + dem.size * 4  # own tables for the shared ones + the staging buffer
        assert {k: val for k, val in first.items() if k != "gpu_resource_bytes"} == {k: val for k, val in created.items() if k != "gpu_resource_bytes"}
        s.render()
        assert s.info() == first
        for i in range(10):
            _apply(s, steps[i % len(steps)])
            assert s.info() == first
        s.render()
        assert s.info() == first
    # the smallest budget (in KiB steps) the create accepts leaves no room for the staging buffer of the whole DEM
    for budget in range(need, need + (64 << 10), 1 << 10):
        try:
            s = _session(dem, cam, kw, memory_budget_bytes=budget, **opts)
            break
        except RuntimeError as e:
            assert "exceeds the memory budget" in str(e)
    else:
        raise AssertionError("no budget accepted")
    with s:
        assert budget < need + dem.size * 4
        want = s.render()
        with pytest.raises(RuntimeError, match="re-terrain exceeds the memory budget"):
            s.reterrain(dem * np.float32(0.9))
        assert s.info()["gpu_resource_bytes"] == need
        s.rearm()
        _same(s.render(), want, "after a re-terrain the budget refused")
        with _session(dem, cam, kw, **opts) as roomy:
            _same(want, roomy.render(), "the old terrain")


def test_refusals_leave_the_session_rendering_the_old_terrain():
    import ctypes as C

    import forge3d_amd as f3d
    from forge3d_amd import _native
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = _golden()
    st = _steps(dem, kw["exaggeration"])[0]
    nan = dem.copy()
    nan[5, 1] = np.nan
    with _session(dem, cam, kw) as s:
        s.reterrain(st["heightmap"], at=st["at"], seed=5)
        state = _state(s)
        want = s.render()
        with pytest.raises(RuntimeError, match="terrain heightfield contains non-finite samples"):  # (status 3, the create's text)
            s.reterrain(nan)
        with pytest.raises(RuntimeError, match="terrain heightfield contains non-finite samples"):
            s.reterrain(np.full((2, 2), np.inf, np.float32), at=(3, 3))
        with pytest.raises(ValueError, match="leaves the session's 64x64 DEM"):
            s.reterrain(np.zeros((4, 4), np.float32), at=(61, 0))
        with pytest.raises(ValueError, match="leaves the session's 64x64 DEM"):
            s.reterrain(np.zeros((1, 1), np.float32), at=(0, 64))
        with pytest.raises(ValueError, match="re-terrain block is empty"):
            s.reterrain(np.zeros((0, 4), np.float32), at=(1, 1))
        with pytest.raises(ValueError, match="a new exaggeration .* rescales every sample"):
            s.reterrain(np.zeros((4, 4), np.float32), at=(1, 1), exaggeration=2.0 * kw["exaggeration"])
        for bad in (-1.0, float("inf"), float("nan"), 0.0):
            with pytest.raises(RuntimeError, match="terrain exaggeration must be finite and > 0"):  # the create's refusal
                s.reterrain(dem, exaggeration=bad)
        with pytest.raises(RuntimeError, match="camera look_at must differ from origin"):  # a camera the create refuses
            s.reterrain(dem, dict(ORBIT, look_at=ORBIT["origin"]))
        t = _native.ReterrainDesc()  # another revision's descriptor
        t.struct_size = C.sizeof(_native.ReterrainDesc) + 8
        err = C.create_string_buffer(512)
        assert _native.lib().f3d_session_reterrain(s._handle, C.byref(t), err, len(err)) == 1
        assert b"f3d_session_reterrain_desc.struct_size" in err.value
        with pytest.raises(ValueError, match="re-arm it"):
            s.render()
        s.rearm()
        assert _state(s) == state
        _same(s.render(), want, "after refused re-terrains")
        _same(want, f3d.hybrid_render_terrain_reference(st["dem"], W, H, cam, **dict(kw, seed=5)), "the old terrain")
    bounds = [(0, 29), (29, 64)]
    sessions = [TerrainSession(dem, W, H, cam, row_begin=b, row_end=e, **kw) for b, e in bounds]
    try:
        exports = [x.halo_export() for x in sessions]
        sessions[0].halo_connect(1, exports[1])
        sessions[1].halo_connect(0, exports[0])
        for x in sessions:
            with pytest.raises(ValueError, match="a session with peer halos cannot be re-terrained"):  # (status 1)
                x.reterrain(dem)
    finally:
        for x in sessions:
            x.close()


_HORIZON_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_reterrain as t
dem, cam, kw = t._golden()
with t._session(dem, cam, kw) as s:
    want = s.render()
    try:
        s.reterrain(dem * np.float32(0.5))
    except ValueError as e:
        assert "far-horizon table" in str(e), str(e)
    else:
        raise AssertionError("accepted")
    s.rearm()
    t._same(s.render(), want, "after the refusal")
print("refused")
"""


def test_a_session_with_the_far_horizon_table_refuses():
    env = dict(os.environ, F3D_IBL_HORIZON="1")
    proc = subprocess.run([sys.executable, "-c", _HORIZON_CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "refused" in proc.stdout, proc.stderr[-3000:]


def test_reterrain_without_a_host_wait_after_frames_and_a_device_resolve_and_after_a_pool_trim():
    import torch

    from forge3d_amd import _native

    dem, cam, kw = _golden()
    dev = torch.device("cuda", 0)
    steps = _steps(dem, kw["exaggeration"])[:8]  # (they keep the 4-frame budget)
    held = _held(cam, kw, steps)
    rgba = [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(len(steps) + 1)]
    with _session(dem, cam, kw, frames_in_flight=0) as s:
        for i in range(len(steps) + 1):
            if i:
                _apply(s, steps[i - 1])  # (behind the frames and the resolve just enqueued)
            s.enqueue_frames(0, 4)
            s.resolve_device(4, d_rgba=rgba[i].data_ptr())
        torch.cuda.synchronize()
        for i, (d, c, k) in enumerate([(dem, cam, kw)] + held):
            with _session(d, c, k, frames_in_flight=0) as fresh:
                assert np.array_equal(rgba[i].cpu().numpy(), fresh.render()["rgba"]), i
        _native.lib().f3d_device_pool_trim()
        _apply(s, steps[0])
        d = dem.copy()
        d[26:38, 26:38] = steps[0]["heightmap"]
        with _session(d, cam, kw, frames_in_flight=0) as fresh:
            _same(s.render(), fresh.render(), "after a trim")


def test_render_terrain_dem_sequence_equals_one_shots():
    import forge3d_amd as f3d
    from forge3d_amd.path_tracing import render_terrain_dem_sequence

    dem, cam, kw = _golden()
    steps = _steps(dem, kw["exaggeration"])
    common = {key: val for key, val in kw.items() if key not in ("sun_azimuth_deg", "sun_elevation_deg")}
    sun = dict(sun_azimuth_deg=225.0, sun_elevation_deg=35.0)
    frames = [dict(sun), dict(sun, heightmap=steps[0]["dem"]), dict(sun, heightmap=steps[1]["dem"], camera=ORBIT),
              dict(camera=ORBIT, sun_azimuth_deg=10.0, sun_elevation_deg=12.0, seed=99, max_frames=3, min_frames=3),  # no heightmap: the positional DEM again
              dict(sun, exaggeration=steps[6]["exag"]),                                                                 # the exaggeration alone
              dict(sun, heightmap=steps[5]["dem"], exaggeration=steps[6]["exag"], sun_color=(0.5, 0.6, 1.0)),
              dict(sun, heightmap=steps[5]["dem"], exaggeration=steps[6]["exag"], seed=3),                              # the DEM stays: a re-aim
              dict(sun, heightmap=-steps[4]["dem"])]
    got = list(render_terrain_dem_sequence(dem, W, H, cam, frames=frames, **common))
    assert len(got) == len(frames)
    for i, frame in enumerate(frames):  # item i is the one-shot on frames[i]["heightmap"] with **common, **rest: a key a frame does not name is common's
        rest = {k: val for k, val in frame.items() if k not in ("camera", "heightmap")}
        want = f3d.hybrid_render_terrain_reference(frame.get("heightmap", dem), W, H, frame.get("camera", cam), **{**common, **rest})
        assert sorted(got[i]) == sorted(want)
        for key in AOVS:
            assert np.array_equal(got[i][key], want[key], equal_nan=True), (i, key)
        for key in SCALARS:
            if key != "gpu_resource_bytes":
                assert got[i][key] == want[key], (i, key)
