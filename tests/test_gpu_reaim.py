"""`-m gpu`: re-aim of a live terrain session (f3d_session_reaim: a re-arm under a new camera), byte for byte against fresh renders.

A re-aimed session must render exactly what a new session (or the one-shot call) renders under the new camera and values:
all four outputs, frames, variance, converged, the certificates and the fingerprint after each re-aim.  A chain of cameras
(an orbit step, a fov change, a view that sees sky only -- which the one-shot refuses under a lit sun, and so must the
re-aimed render, leaving the session re-aimable --, a normal view, sun and seed changing along the way) over the session
forms (fused frames, frames in flight, bands on several streams, 1 / 4 / 8 sample lanes), with meshes of both builders, the
AETHER post (camera height and pixel rays change), curvature on a small sphere; re-aimed row strips; a re-aim enqueued
behind frames and a resolve without a host wait; after a pool trim and a scene-cache eviction; the memory it must not take;
refused cameras; the chain under every poison pattern of the allocator (in child processes); a session with peer halos;
and the Python forms on top: render_terrain_camera_sequence and ViewerHandle.render_animation through one session.
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

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
AOVS = ("rgba", "albedo", "normal", "depth")
SCALARS = ("frames", "variance", "converged", "gpu_resource_bytes", "minmax_pyramid_bytes", "peak_host_visible_bytes",
           "sun_source", "solar_azimuth_deg", "solar_elevation_deg")
AUTO = 0xFFFFFFFF
W, H = 96, 64

ORBIT = {"origin": (63.6, 35.0, 63.6), "look_at": (0.0, 5.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}
SKY = {"origin": (0.0, 60.0, 0.0), "look_at": (5.0, 160.0, 0.0), "up": (0.0, 0.0, 1.0), "fov_y": 40.0}
# the chain: (camera, re-armable values given with it); the camera dict is read as the constructor reads it
CHAIN = [
    (ORBIT, {}),                                                                     # an orbit step, nothing else
    (dict(ORBIT, fov_y=28.0), dict(seed=11)),                                        # the fov alone (and a seed)
    (SKY, {}),                                                                       # sky only, the sun lit: refused by the render
    ({"origin": (-70.0, 45.0, 40.0), "look_at": (0.0, 8.0, 5.0), "up": (0.1, 1.0, 0.0), "fov_y": 50.0, "exposure": 1.6},
     dict(sun_azimuth_deg=80.0, sun_elevation_deg=20.0, max_frames=3, min_frames=3)),    # camera AND sun in one call
    (SKY, dict(sun_elevation_deg=-4.0)),                                             # sky only under a set sun: renders
    ({"origin": (10.0, 80.0, 20.0), "look_at": (10.0, 0.0, 19.0), "fov_y": 60.0},   # steep, default up and exposure
     dict(sun_azimuth_deg=300.0, sun_elevation_deg=55.0, sun_color=(0.9, 0.5, 0.2), env_intensity=0.8, seed=3)),
]


def _golden():
    dem = scenes.golden_dem(4)
    return dem, dict(scenes.CAM), scenes.fixed_frames(scenes.scene_kwargs(dem), 4)


def _held(kw, chain):
    """(camera, render keywords) of every step: a re-aim keeps every re-armable value it is not given, the camera it replaces."""
    held, out = dict(kw), []
    for cam, change in chain:
        held = {**held, **change}
        out.append((dict(cam), held))
    return out


def _same(got, want, what=""):
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key}"
    for key in SCALARS:
        if key in want:
            assert got[key] == want[key], f"{what}: {key} {got[key]!r} != {want[key]!r}"


def _session(dem, cam, kw, **opts):
    from forge3d_amd.session import TerrainSession

    opts.setdefault("frames_in_flight", AUTO)
    return TerrainSession(dem, W, H, cam, **opts, **kw)


def _outcome(call):
    """A render's result, or the (type, message) it was refused with."""
    try:
        return call()
    except (RuntimeError, ValueError) as e:
        return type(e), str(e)


def _same_outcome(got, want, what):
    if isinstance(want, tuple):
        assert got == want, f"{what}: {got!r} instead of the refusal {want!r}"
    else:
        assert not isinstance(got, tuple), f"{what}: refused with {got!r}"
        _same(got, want, what)


def _state(s):
    fp = s.fingerprint()
    if s.frames_in_flight() == 0 and s.sample_lanes() > 1:
        # (the head records of a fused session are written by every frame's head kernel before they are read: a new
        # session leaves them as the allocator hands them out)
        fp.pop("frame_heads")
    return fp, s.certificates()


def _chain(dem, cam, kw, oneshot=True, chain=CHAIN, **opts):
    """Re-aim one session along the chain; every step against a fresh session (and the one-shot) under the same values."""
    import forge3d_amd as f3d

    s = _session(dem, cam, kw, **opts)
    out = []
    try:
        for i, ((camera, change), (c, k)) in enumerate(zip(chain, _held(kw, chain))):
            s.reaim(camera, **change)
            with _session(dem, c, k, **opts) as fresh:
                got_state, want_state = _state(s), _state(fresh)
                assert got_state[0]["gbuffer"] == want_state[0]["gbuffer"], f"step {i}: G-buffer"
                assert got_state[1] == want_state[1], f"step {i}: certificates"
                assert got_state[0] == want_state[0], f"step {i}: fingerprint"
                want = _outcome(fresh.render)
            got = _outcome(s.render)
            _same_outcome(got, want, f"step {i} vs a fresh session")
            if oneshot:
                _same_outcome(got, _outcome(lambda: f3d.hybrid_render_terrain_reference(dem, W, H, c, **k)), f"step {i} vs the one-shot")
            out.append(got)
    finally:
        s.close()
    return out


def test_chain_on_the_golden_dem_equals_one_shots_and_the_oracle():
    from oracle import oracle

    dem, cam, kw = _golden()
    got = _chain(dem, cam, kw)
    assert got[2] == (RuntimeError, got[2][1]) and "no valid reservoirs" in got[2][1]  # sky only under a lit sun, as the reference
    assert not isinstance(got[4], tuple) and np.isnan(got[4]["depth"]).all()            # ... and rendered under a set one
    assert [isinstance(g, tuple) for g in got] == [False, False, True, False, False, False]
    steps = _held(kw, CHAIN)
    for i in (0, 1, 3, 5):  # and the CPU oracle
        c, k = steps[i]
        want = oracle.render(dem, W, H, c, **k)
        for key in AOVS:
            assert np.array_equal(got[i][key], want[key], equal_nan=True), (i, key)
    assert not np.array_equal(got[0]["rgba"], got[1]["rgba"])  # (the fov alone changes the image)


@pytest.mark.parametrize("opts", [dict(frames_in_flight=0), dict(frames_in_flight=4), dict(frames_in_flight=0, bands=3, band_streams=2)],
                         ids=["fused", "in-flight-4", "bands"])
def test_chain_across_session_forms(opts):
    dem, cam, kw = _golden()
    _chain(dem, cam, kw, oneshot=False, **opts)


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_chain_across_sample_lanes(lanes):
    from forge3d_amd.session import kernel_variant

    dem, cam, kw = _golden()
    _chain(dem, cam, dict(kw, spp=8), oneshot=False, frames_in_flight=0, kernel_variant=kernel_variant(sample_lanes=lanes))


@pytest.mark.parametrize("builder", [1, 2], ids=["host-bvh", "gpu-lbvh"])
def test_chain_with_a_mesh(builder):
    dem, cam, kw = _golden()
    v, i = scenes.box_city(n_boxes=30, seed=5)
    kw = dict(kw, mesh_vertices=v, mesh_indices=i)
    _chain(dem, cam, kw, oneshot=builder == 1, mesh_builder=builder)


def test_chain_with_the_aether_post():
    """Camera height and pixel rays enter the aerial-perspective post: a stale camera term shows here."""
    import forge3d_amd as f3d
    from forge3d_amd import _native

    dem, cam, kw = _golden()
    handle = _native._resolve_atmosphere({"turbidity": 3.0})
    s = _session(dem, cam, dict(kw, atmosphere=handle))
    images = []
    try:
        for i, ((camera, change), (c, k)) in enumerate(zip(CHAIN, _held(kw, CHAIN))):
            s.reaim(camera, **change)
            got = _outcome(s.render)
            _same_outcome(got, _outcome(lambda: f3d.hybrid_render_terrain_reference(dem, W, H, c, atmosphere={"turbidity": 3.0}, **k)),
                          f"aether step {i}")
            images.append(got)
    finally:
        s.close()
    c, k = _held(kw, CHAIN)[5]
    plain = f3d.hybrid_render_terrain_reference(dem, W, H, c, **k)
    assert not np.array_equal(images[5]["rgba"], plain["rgba"])  # (the post is on)


def test_chain_with_curvature_on_a_small_sphere():
    dem, cam, kw = _golden()
    kw = dict(kw, earth_model="sphere", refraction_model="none", sphere_radius_m=300.0)
    got = _chain(dem, cam, kw)
    flat = _chain(dem, cam, dict(kw, earth_model="flat"), oneshot=False, chain=CHAIN[:1])
    assert not np.array_equal(got[0]["rgba"], flat[0]["rgba"])  # (the curvature is on)


def test_reaim_without_a_camera_is_a_rearm():
    dem, cam, kw = _golden()
    change = dict(sun_azimuth_deg=80.0, sun_elevation_deg=20.0, seed=11, exposure=1.7)
    with _session(dem, cam, kw) as a, _session(dem, cam, kw) as b:
        a.reaim(**change)
        b.rearm(**change)
        assert _state(a) == _state(b)
        _same(a.render(), b.render(), "reaim() without a camera")
        # exposure: the keyword wins over the camera dict's, the dict's over the default
        a.reaim(dict(ORBIT, exposure=0.5), exposure=1.7)
        b.reaim(dict(ORBIT, exposure=1.7))
        _same(a.render(), b.render(), "exposure keyword")
        a.reaim({k: v for k, v in ORBIT.items() if k != "exposure"})
        b.reaim(ORBIT, exposure=1.0)
        _same(a.render(), b.render(), "default exposure")
        with pytest.raises(TypeError, match="unexpected keyword argument 'spp'"):
            a.reaim(ORBIT, spp=4)


def test_reaim_without_a_host_wait_after_frames_and_a_device_resolve():
    import torch

    dem, cam, kw = _golden()
    dev = torch.device("cuda", 0)
    chain = [CHAIN[0], CHAIN[1], CHAIN[5]]  # (three re-aims that keep the 4-frame budget)
    rgba = [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(len(chain) + 1)]
    with _session(dem, cam, kw, frames_in_flight=0) as s:
        for i in range(len(chain) + 1):
            if i:
                s.reaim(chain[i - 1][0], **chain[i - 1][1])  # (behind the frames and the resolve just enqueued: no synchronisation)
            s.enqueue_frames(0, 4)
            s.resolve_device(4, d_rgba=rgba[i].data_ptr())
        torch.cuda.synchronize()
        for i, (c, k) in enumerate([(cam, kw)] + _held(kw, chain)):
            with _session(dem, c, k, frames_in_flight=0) as fresh:
                assert np.array_equal(rgba[i].cpu().numpy(), fresh.render()["rgba"]), i


def test_reaim_after_a_pool_trim_and_a_scene_cache_eviction():
    from forge3d_amd import _native

    L = _native.lib()
    dem, cam, kw = _golden()
    v, i = scenes.box_city(n_boxes=12, seed=9)
    kw = dict(kw, mesh_vertices=v, mesh_indices=i)
    steps = _held(kw, CHAIN)
    s = _session(dem, cam, kw)
    try:
        s.render()
        L.f3d_device_pool_trim()
        s.reaim(CHAIN[0][0], **CHAIN[0][1])
        with _session(dem, *steps[0]) as fresh:
            _same(s.render(), fresh.render(), "after a trim")
        L.f3d_scene_cache_limit(0)  # the session's tables and mesh leave the cache while it lives
        try:
            s.reaim(CHAIN[1][0], **CHAIN[1][1])
            got = s.render()
        finally:
            L.f3d_scene_cache_limit(2)
        with _session(dem, *steps[1]) as fresh:
            _same(got, fresh.render(), "after an eviction")
    finally:
        s.close()


@pytest.mark.parametrize("in_flight", [0, 4])
def test_reaimed_row_strips_equal_the_whole_image(in_flight):
    """Two strips with caller-owned reservoirs and the device-copy halo exchange (as test_gpu_rearm's strip test)."""
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

    chain = [CHAIN[0], CHAIN[1], CHAIN[3], CHAIN[5]]
    try:
        render(4)
        for i, ((camera, change), (c, k)) in enumerate(zip(chain, _held(kw, chain))):
            for s in sessions:
                s.reaim(camera, **change)
            got = render(int(k["max_frames"]))
            want = f3d.hybrid_render_terrain_reference(dem, W, H, c, **k)
            for key in AOVS:
                assert np.array_equal(got[key], want[key], equal_nan=True), (i, key)
    finally:
        for s in sessions:
            s.close()


def test_ten_reaims_take_no_memory():
    dem, cam, kw = _golden()
    with _session(dem, cam, kw) as s:
        s.render()
        before = s.info()
        pointer = s.primary_start_ptr()
        for i in range(10):
            ang = 0.3 * i
            s.reaim(dict(ORBIT, origin=(90.0 * np.sin(ang), 35.0, 90.0 * np.cos(ang))), seed=i)
            assert s.info() == before
            assert s.primary_start_ptr() == pointer
        s.render()
        assert s.info() == before


def test_a_refused_camera_leaves_the_session_rendering_the_old_view():
    import forge3d_amd as f3d

    dem, cam, kw = _golden()
    bad = [dict(ORBIT, look_at=ORBIT["origin"]), dict(ORBIT, origin=(0.0, float("nan"), 1.0)), dict(ORBIT, origin=(float("inf"), 0.0, 1.0)),
           dict(ORBIT, up=(0.0, 0.0, 0.0)), dict(ORBIT, fov_y=180.0), dict(SKY, look_at=(0.0, 160.0, 0.0), up=(0.0, 1.0, 0.0))]
    with _session(dem, cam, kw) as s:
        s.reaim(ORBIT, seed=5)
        state = _state(s)
        want = s.render()
        for camera in bad:
            with pytest.raises(RuntimeError) as one_shot:
                f3d.hybrid_render_terrain_reference(dem, W, H, camera, **kw)
            with pytest.raises(RuntimeError) as reaim:
                s.reaim(camera, sun_azimuth_deg=10.0)
            assert str(reaim.value) == str(one_shot.value)
        with pytest.raises(ValueError, match="re-arm it"):
            s.render()  # (its state is spent: a new render needs a re-arm or a re-aim)
        s.rearm()  # (no values: the session's own again -- the camera and the sun of the last accepted re-aim)
        assert _state(s) == state
        _same(s.render(), want, "after refused cameras")
        _same(want, f3d.hybrid_render_terrain_reference(dem, W, H, ORBIT, **dict(kw, seed=5)), "the old view")
        c, k = _held(kw, CHAIN[3:4])[0]
        s.reaim(CHAIN[3][0], **CHAIN[3][1])
        _same(s.render(), f3d.hybrid_render_terrain_reference(dem, W, H, c, **dict(k, seed=5)), "re-aimed after a refusal")


def test_a_session_with_peer_halos_refuses_a_reaim():
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = _golden()
    bounds = [(0, 29), (29, 64)]
    sessions = [TerrainSession(dem, W, H, cam, row_begin=b, row_end=e, **kw) for b, e in bounds]
    try:
        exports = [s.halo_export() for s in sessions]
        sessions[0].halo_connect(1, exports[1])
        sessions[1].halo_connect(0, exports[0])
        for s in sessions:
            with pytest.raises(ValueError, match="a session with peer halos cannot be re-aimed"):  # (status 1)
                s.reaim(ORBIT)
    finally:
        for s in sessions:
            s.close()


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_reaim as t
dem, cam, kw = t._golden()
v, i = t.scenes.box_city(n_boxes=12, seed=9)
out = {}
for name, k, opts in (("plain", kw, {}), ("fused", kw, {"frames_in_flight": 0}), ("mesh", dict(kw, mesh_vertices=v, mesh_indices=i), {})):
    s = t._session(dem, cam, k, **opts)
    for j, (camera, change) in enumerate(t.CHAIN):
        s.reaim(camera, **change)
        r = t._outcome(s.render)
        if isinstance(r, tuple):
            out[f"{name}_{j}_refused"] = np.frombuffer(r[1].encode(), np.uint8)
            continue
        for key in t.AOVS:
            out[f"{name}_{j}_{key}"] = r[key]
    s.close()
np.savez(sys.argv[2], **out)
"""


def _chain_in_child(poison, path):
    env = dict(os.environ)
    env.pop("F3D_POISON", None)
    if poison is not None:
        env["F3D_POISON"] = str(poison)
    proc = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    return dict(np.load(path))


def test_the_chain_under_every_poison_pattern_equals_the_plain_run():
    """What a re-aim must clear or rewrite is whatever a new session's create clears or writes: with the allocator filling
    every buffer with a pattern (f3d_debug_poison), a state the re-aim forgets would carry the pattern (or the last view)
    into the next render."""
    with tempfile.TemporaryDirectory() as tmp:
        plain = _chain_in_child(None, Path(tmp) / "plain.npz")
        assert len(plain) == 3 * (5 * len(AOVS) + 1)
        for pattern in (0, 0x5A, 0xFF):
            got = _chain_in_child(pattern, Path(tmp) / f"p{pattern}.npz")
            assert sorted(got) == sorted(plain)
            for key in plain:
                assert np.array_equal(got[key], plain[key], equal_nan=True), (pattern, key)


def test_render_terrain_camera_sequence_equals_one_shots():
    import forge3d_amd as f3d
    from forge3d_amd.geo import SolarTime
    from forge3d_amd.path_tracing import render_terrain_camera_sequence

    dem, cam, kw = _golden()
    common = {key: v for key, v in kw.items() if key not in ("sun_azimuth_deg", "sun_elevation_deg")}
    when = SolarTime(utc=(2024, 6, 21, 17, 0, 0), observer_lat=46.85, observer_lon=-121.76, observer_elev_m=1500.0, tz_offset_hours=-7.0,
                     delta_t_seconds=69.0, pressure_mbar=850.0, temperature_c=10.0)
    frames = [dict(camera=cam, sun_azimuth_deg=225.0, sun_elevation_deg=35.0), dict(camera=ORBIT, sun_azimuth_deg=225.0, sun_elevation_deg=35.0),
              dict(camera=dict(ORBIT, fov_y=30.0, exposure=1.4), solar_time=when),
              dict(camera={"origin": (-70.0, 45.0, 40.0)}, sun_azimuth_deg=10.0, sun_elevation_deg=12.0, seed=99, max_frames=3, min_frames=3),
              dict(camera=SKY, sun_azimuth_deg=10.0, sun_elevation_deg=-3.0),
              dict(camera=CHAIN[5][0], sun_azimuth_deg=11.0, sun_elevation_deg=89.0, sun_color=(0.5, 0.6, 1.0), env_intensity=0.9)]
    got = list(render_terrain_camera_sequence(dem, W, H, frames=frames, **common))
    assert len(got) == len(frames)
    for i, frame in enumerate(frames):
        rest = {k: v for k, v in frame.items() if k != "camera"}
        want = f3d.hybrid_render_terrain_reference(dem, W, H, frame["camera"], **{**common, **rest})
        assert sorted(got[i]) == sorted(want)
        _same(got[i], want, f"sequence frame {i}")
        assert got[i]["sun_source"] == ("solar_time" if "solar_time" in frame else "manual_angles")
    # a frame the render refuses ends the sequence there with the one-shot's refusal, after the frames before it
    lit_sky = [frames[1], dict(camera=SKY, sun_azimuth_deg=225.0, sun_elevation_deg=35.0), frames[0]]
    sequence = render_terrain_camera_sequence(dem, W, H, frames=lit_sky, **common)
    _same(next(sequence), got[1], "before the refused frame")
    with pytest.raises(RuntimeError) as one_shot:
        f3d.hybrid_render_terrain_reference(dem, W, H, SKY, **{**common, "sun_azimuth_deg": 225.0, "sun_elevation_deg": 35.0})
    with pytest.raises(RuntimeError) as refused:
        next(sequence)
    assert str(refused.value) == str(one_shot.value)


def test_the_viewers_animation_renders_through_one_session(tmp_path, monkeypatch):
    import forge3d_amd as f3d
    from forge3d_amd import _native, io
    from forge3d_amd.datasets import orbit_camera

    dem = (scenes.golden_dem() * 20.0).astype(np.float32)
    spacing = scenes.SPAN / (dem.shape[1] - 1)
    L = _native.lib()
    L.f3d_scene_cache_limit(0)
    L.f3d_scene_cache_limit(2)
    h = f3d.open_viewer_async(W, H, fov_deg=45.0)
    h.load_terrain(dem, spacing)
    h._render.update(spp=2, max_frames=3, min_frames=3, variance_threshold=1e30)
    h.set_sun(225.0, 35.0)
    keys = [dict(phi_deg=20.0, theta_deg=60.0, radius=110.0, target=(0.0, 5.0, 0.0)), dict(phi_deg=50.0, theta_deg=60.0, radius=110.0, target=(0.0, 5.0, 0.0)),
            dict(phi_deg=80.0, theta_deg=40.0, radius=90.0, fov_deg=30.0, target=(0.0, 5.0, 0.0)), dict(phi_deg=110.0, theta_deg=60.0, radius=110.0)]
    creates, seen = [], []
    create = L.f3d_session_create

    def counted(*args):
        creates.append(1)
        return create(*args)

    monkeypatch.setattr(L, "f3d_session_create", counted)
    h.render_animation(keys, tmp_path / "frames", progress_callback=lambda i, n: seen.append((i, n)))
    monkeypatch.undo()
    assert len(creates) == 1 and L.f3d_scene_cache_entries() == 1
    assert seen == [(i, len(keys)) for i in range(len(keys))]
    fov = 45.0
    for i, k in enumerate(keys):
        fov = k.get("fov_deg", fov)
        target = k.get("target", (0.0, 0.5 * float(dem.max()), 0.0))
        cam = orbit_camera(target, k["radius"], k["phi_deg"], k["theta_deg"], fov)
        want = f3d.hybrid_render_terrain_reference(dem, W, H, cam, spacing=(spacing, spacing), sun_azimuth_deg=225.0, sun_elevation_deg=35.0,
                                                   spp=2, max_frames=3, min_frames=3, variance_threshold=1e30)
        assert np.array_equal(io.png_to_numpy(tmp_path / "frames" / f"frame_{i:04d}.png"), want["rgba"]), i
    assert sorted(h.last_result) == sorted(want) and h.get_stats()["frames"] == 3
    _same(h.last_result, want, "last_result")
    h.snapshot(tmp_path / "snap.png")  # (the handle still renders on its own afterwards)
    assert np.array_equal(io.png_to_numpy(tmp_path / "snap.png"), want["rgba"])
