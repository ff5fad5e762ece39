"""`-m gpu`: re-arm of a live terrain session (f3d_session_rearm / f3d_session_render), byte for byte against fresh renders.

A re-armed session must render exactly what a new session (or the one-shot call) renders with the new sun, seed, exposure,
IBL intensity and frame budget: chains of re-arms over several scene forms (golden DEM, rainier proxy, meshes of both
builders, 1 / 4 / 8 sample lanes, frames in flight and fused frames, bands on several streams, the AETHER post), the
session's fingerprint and certificates after each re-arm, a re-arm enqueued behind frames and a resolve without a host
wait, re-arms after a pool trim and a scene-cache eviction, row strips with caller-owned reservoirs, the memory a re-arm
must not take, a refused sun, the chain under every poison pattern of the allocator (in child processes), and the two
Python forms on top: render_terrain_sequence and the smoke sequence's terrain provider.
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

# the chain: sun azimuth / elevation (the zenith and below the horizon), intensity and colour, seed, exposure, IBL, budget
CHAIN = [
    dict(sun_azimuth_deg=80.0, sun_elevation_deg=20.0, seed=11),
    dict(sun_azimuth_deg=80.25, sun_elevation_deg=90.0, sun_intensity=4.0, max_frames=3, min_frames=3),
    dict(sun_azimuth_deg=300.0, sun_elevation_deg=-6.0, sun_color=(0.9, 0.5, 0.2), env_intensity=0.8, seed=3),
    dict(sun_azimuth_deg=135.0, sun_elevation_deg=8.0, exposure=1.7, max_frames=5, min_frames=5, env_intensity=0.1),
    dict(sun_azimuth_deg=135.5, sun_elevation_deg=55.0, sun_intensity=0.0, seed=12345),
]


def _fixed(kw, frames=4):
    return scenes.fixed_frames(kw, frames)


def _golden():
    dem = scenes.golden_dem(4)
    return dem, dict(scenes.CAM), _fixed(scenes.scene_kwargs(dem), 4)


def _cumulative(changes):
    """What the session holds after each re-arm of `changes` (a re-arm keeps every value it is not given)."""
    held, out = {}, []
    for change in changes:
        held = {**held, **change}
        out.append(held)
    return out


def _merge(kw, cam, change):
    """(render keywords, camera) of a chain step: exposure lives in the camera dict."""
    k, c = dict(kw), dict(cam)
    for key, v in change.items():
        if key == "exposure":
            c["exposure"] = v
        else:
            k[key] = v
    return k, c


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


def _fresh(dem, cam, kw, **opts):
    with _session(dem, cam, kw, **opts) as s:
        return s.render()


def _chain(dem, cam, kw, oneshot=True, check_state=False, **opts):
    """Re-arm one session along CHAIN; every step against a fresh session (and the one-shot) with those values."""
    import forge3d_amd as f3d

    s = _session(dem, cam, kw, **opts)
    out = []
    try:
        for i, (change, held) in enumerate(zip(CHAIN, _cumulative(CHAIN))):
            k, c = _merge(kw, cam, held)
            s.rearm(**change)
            if check_state:
                with _session(dem, c, k, **opts) as fresh:
                    want_fp, got_fp = fresh.fingerprint(), s.fingerprint()
                    if fresh.frames_in_flight() == 0 and fresh.sample_lanes() > 1:
                        # (the head records of a fused session are written by every frame's head kernel before they are read:
                        # a new session leaves them as the allocator hands them out)
                        want_fp.pop("frame_heads"), got_fp.pop("frame_heads")
                    assert got_fp == want_fp, f"step {i}: fingerprint"
                    assert s.certificates() == fresh.certificates(), f"step {i}: certificates"
            got = s.render()
            _same(got, _fresh(dem, c, k, **opts), f"step {i} vs a fresh session")
            if oneshot:
                _same(got, f3d.hybrid_render_terrain_reference(dem, W, H, c, **k), f"step {i} vs the one-shot")
            out.append(got)
    finally:
        s.close()
    return out


def test_chain_on_the_golden_dem_equals_one_shots_and_the_oracle():
    from oracle import oracle

    dem, cam, kw = _golden()
    got = _chain(dem, cam, kw, check_state=True)
    for i in (0, 2):  # and the CPU oracle
        k, c = _merge(kw, cam, _cumulative(CHAIN)[i])
        want = oracle.render(dem, W, H, c, **k)
        for key in AOVS:
            assert np.array_equal(got[i][key], want[key], equal_nan=True), (i, key)


@pytest.mark.parametrize("opts", [dict(frames_in_flight=0), dict(frames_in_flight=4), dict(frames_in_flight=0, bands=3, band_streams=2)],
                         ids=["fused", "in-flight-4", "bands"])
def test_chain_across_session_forms(opts):
    dem, cam, kw = _golden()
    _chain(dem, cam, kw, oneshot=False, check_state=True, **opts)


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_chain_across_sample_lanes(lanes):
    from forge3d_amd.session import kernel_variant

    dem, cam, kw = _golden()
    _chain(dem, cam, dict(kw, spp=8), oneshot=False, check_state=True, frames_in_flight=0, kernel_variant=kernel_variant(sample_lanes=lanes))


@pytest.mark.parametrize("builder", [1, 2], ids=["host-bvh", "gpu-lbvh"])
def test_chain_with_a_mesh(builder):
    dem, cam, kw = _golden()
    v, i = scenes.box_city(n_boxes=30, seed=5)
    kw = dict(kw, mesh_vertices=v, mesh_indices=i)
    _chain(dem, cam, kw, oneshot=builder == 1, check_state=True, mesh_builder=builder)


def test_chain_on_a_reduced_rainier_proxy():
    from forge3d_amd import datasets

    dem, cam, kw = datasets.rainier_proxy_scene(256)
    kw = _fixed(dict(kw, spp=2), 3)
    _chain(dem, dict(cam), kw)


def test_chain_with_the_aether_post():
    from forge3d_amd import _native

    dem, cam, kw = _golden()
    import forge3d_amd as f3d

    handle = _native._resolve_atmosphere({"turbidity": 3.0})
    s = _session(dem, cam, dict(kw, atmosphere=handle))
    try:
        for i, (change, held) in enumerate(zip(CHAIN[:4], _cumulative(CHAIN[:4]))):
            k, c = _merge(kw, cam, held)
            s.rearm(**change)
            _same(s.render(), f3d.hybrid_render_terrain_reference(dem, W, H, c, atmosphere={"turbidity": 3.0}, **k), f"aether step {i}")
    finally:
        s.close()


def test_rearm_without_a_host_wait_after_frames_and_a_device_resolve():
    import torch

    dem, cam, kw = _golden()
    dev = torch.device("cuda", 0)
    rgba = [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(3)]
    changes = [{}, CHAIN[2], CHAIN[4]]  # (the create's values, then two re-arms that keep the 4-frame budget)
    with _session(dem, cam, kw, frames_in_flight=0) as s:
        for i, change in enumerate(changes):
            if i:
                s.rearm(**change)  # (behind the frames and the resolve just enqueued: no synchronisation in between)
            s.enqueue_frames(0, 4)
            s.resolve_device(4, d_rgba=rgba[i].data_ptr())
        torch.cuda.synchronize()
        for i, held in enumerate(_cumulative(changes)):
            k, c = _merge(kw, cam, held)
            assert np.array_equal(rgba[i].cpu().numpy(), _fresh(dem, c, k, frames_in_flight=0)["rgba"]), i


def test_rearm_after_a_pool_trim_and_a_scene_cache_eviction():
    from forge3d_amd import _native

    L = _native.lib()
    dem, cam, kw = _golden()
    v, i = scenes.box_city(n_boxes=12, seed=9)
    kw = dict(kw, mesh_vertices=v, mesh_indices=i)
    s = _session(dem, cam, kw)
    try:
        s.render()
        L.f3d_device_pool_trim()
        k, c = _merge(kw, cam, CHAIN[1])
        s.rearm(**CHAIN[1])
        _same(s.render(), _fresh(dem, c, k), "after a trim")
        L.f3d_scene_cache_limit(0)  # the session's tables and mesh leave the cache while it lives
        try:
            s.rearm(**CHAIN[2])
            got = s.render()
        finally:
            L.f3d_scene_cache_limit(2)
        k, c = _merge(kw, cam, {**CHAIN[1], **CHAIN[2]})
        _same(got, _fresh(dem, c, k), "after an eviction")
    finally:
        s.close()


@pytest.mark.parametrize("in_flight", [0, 4])
def test_rearmed_row_strips_equal_the_whole_image(in_flight):
    """Two strips with caller-owned reservoirs and the device-copy halo exchange (as test_gpu_parity's strip test)."""
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

    try:
        render(4)
        for i, (change, held) in enumerate(zip(CHAIN[1:4], _cumulative(CHAIN[1:4]))):
            k, c = _merge(kw, cam, held)
            for s in sessions:
                s.rearm(**change)
            frames = int(k["max_frames"])
            got = render(frames)
            want = f3d.hybrid_render_terrain_reference(dem, W, H, c, **k)
            for key in AOVS:
                assert np.array_equal(got[key], want[key], equal_nan=True), (i, key)
    finally:
        for s in sessions:
            s.close()


def test_ten_rearms_take_no_memory():
    dem, cam, kw = _golden()
    with _session(dem, cam, kw) as s:
        s.render()
        before = s.info()
        for i in range(10):
            s.rearm(sun_azimuth_deg=10.0 * i, seed=i)
            assert s.info() == before
        s.render()
        assert s.info() == before


def test_a_non_finite_sun_is_refused_and_the_session_still_renders():
    import forge3d_amd as f3d

    dem, cam, kw = _golden()
    with pytest.raises(RuntimeError) as one_shot:
        f3d.hybrid_render_terrain_reference(dem, W, H, cam, **dict(kw, sun_azimuth_deg=float("nan")))
    with _session(dem, cam, kw) as s:
        s.render()
        with pytest.raises(RuntimeError) as rearm:
            s.rearm(sun_azimuth_deg=float("nan"))
        assert str(rearm.value) == str(one_shot.value)
        with pytest.raises(ValueError, match="sun_color"):
            s.rearm(sun_color=(1.0, float("inf"), 0.0))
        with pytest.raises(ValueError, match="re-arm it"):
            s.render()  # (its state is spent: a new render needs a re-arm)
        s.rearm()  # (no values: the session's own again)
        _same(s.render(), f3d.hybrid_render_terrain_reference(dem, W, H, cam, **kw), "after a refused re-arm")
        k, c = _merge(kw, cam, CHAIN[2])
        s.rearm(**CHAIN[2])
        _same(s.render(), f3d.hybrid_render_terrain_reference(dem, W, H, c, **k), "re-armed after a refusal")


_CHILD = r"""
import sys, json
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_rearm as t
from forge3d_amd import _native
dem, cam, kw = t._golden()
v, i = t.scenes.box_city(n_boxes=12, seed=9)
out = {}
for name, k, opts in (("plain", kw, {}), ("fused", kw, {"frames_in_flight": 0}), ("mesh", dict(kw, mesh_vertices=v, mesh_indices=i), {})):
    s = t._session(dem, cam, k, **opts)
    for j, change in enumerate(t.CHAIN):
        s.rearm(**change)
        r = s.render()
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
    """What a re-arm must clear is whatever a new session's create clears: with the allocator filling every buffer with a
    pattern (f3d_debug_poison), a state the re-arm forgets would carry the pattern (or the last render) into the next."""
    with tempfile.TemporaryDirectory() as tmp:
        plain = _chain_in_child(None, Path(tmp) / "plain.npz")
        for pattern in (0, 0x5A, 0xFF):
            got = _chain_in_child(pattern, Path(tmp) / f"p{pattern}.npz")
            assert sorted(got) == sorted(plain)
            for key in plain:
                assert np.array_equal(got[key], plain[key], equal_nan=True), (pattern, key)


def test_render_terrain_sequence_equals_one_shots():
    import forge3d_amd as f3d
    from forge3d_amd.geo import SolarTime
    from forge3d_amd.path_tracing import render_terrain_sequence

    dem, cam, kw = _golden()
    common = {key: v for key, v in kw.items() if key not in ("sun_azimuth_deg", "sun_elevation_deg")}
    when = [SolarTime(utc=(2024, 6, 21, h, 0, 0), observer_lat=46.85, observer_lon=-121.76, observer_elev_m=1500.0, tz_offset_hours=-7.0,
                      delta_t_seconds=69.0, pressure_mbar=850.0, temperature_c=10.0) for h in (17, 22)]
    frames = [dict(sun_azimuth_deg=225.0, sun_elevation_deg=35.0), dict(solar_time=when[0]),
              dict(sun_azimuth_deg=225.25, sun_elevation_deg=35.0, seed=99), dict(solar_time=when[1], sun_intensity=3.0),
              dict(sun_azimuth_deg=10.0, sun_elevation_deg=-3.0, max_frames=3, min_frames=3),
              dict(sun_azimuth_deg=11.0, sun_elevation_deg=89.0, sun_color=(0.5, 0.6, 1.0), env_intensity=0.9)]
    got = list(render_terrain_sequence(dem, W, H, cam, frames=frames, **common))
    assert len(got) == 6
    for i, frame in enumerate(frames):
        want = f3d.hybrid_render_terrain_reference(dem, W, H, cam, **{**common, **frame})
        assert sorted(got[i]) == sorted(want)
        _same(got[i], want, f"sequence frame {i}")
        assert got[i]["sun_source"] == ("solar_time" if "solar_time" in frame else "manual_angles")


def test_the_smoke_providers_frames_equal_a_new_session_per_frame():
    import torch

    from forge3d_amd import smoke
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = _golden()
    render = {key: v for key, v in kw.items() if key not in ("max_frames", "min_frames", "variance_threshold", "sun_azimuth_deg")}
    dims, n = (24, 16, 20), 4
    view = dict(camera_pos=(12.0, 10.0, 46.0), target=(12.0, 6.0, 10.0))
    emitters = [smoke.SmokeEmitter(center=(6.0, 3.0, 10.0), radius=2.5, density_rate=6.0, temperature_rate=3.0, soot_rate=0.3,
                                   emission_rate=2.0, velocity=(3.0, 0.4, 0.0))]
    settings = smoke.SmokeStepSettings(dt=0.1, turbulence_strength=0.5, turbulence_seed=7, wind=(1.5, 0.0, -0.2), pressure_iterations=8)
    terrain = np.zeros((H, W, 4), np.uint8)

    def sun(i):
        return {"sun_azimuth_deg": 225.0 + 0.25 * (i + 1)}

    def run(provider):
        seq = smoke.SmokeSequence(smoke.SmokeDomain(dims), terrain, **view)
        return [np.array(f) for f in seq.frames(n, settings, emitters, base_provider=provider)]

    provider = smoke.terrain_sun_provider(dem, cam, sun_path=sun, frames=4, **render)
    try:
        got = run(provider)
    finally:
        provider.close()
    held = []

    def fresh(i, base, stream):
        s = TerrainSession(dem, W, H, cam, stream=stream.cuda_stream, max_frames=4, min_frames=4, **render, **sun(i))
        s.enqueue_frames(0, 4)
        s.resolve_device(4, d_rgba=base.data_ptr())
        held.append(s)

    want = run(fresh)
    torch.cuda.synchronize()
    for s in held:
        s.close()
    assert len(got) == len(want) == n
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i
