"""`-m gpu`: re-mesh of a live terrain session (f3d_session_remesh: a re-aim under a moved or another mesh), byte for byte
against fresh renders.

Images do not depend on the mesh's tree -- the answer is the sweep's, the BVH only culls -- so a session whose BVH was
refitted on the GPU after its vertices moved must render exactly what a new session (or the one-shot call, or the CPU
oracle) renders with the moved mesh: all four outputs, frames, variance, converged, both certificates, and every
fingerprint entry but the tree's own.  A chain of motions (a rigid shift, per-vertex jitter, the positions permuted across
the scene, every vertex collapsed to one point, the mesh 10^4 units away, back to the original, and camera + sun + mesh in
one call) over the three builders (host SAH walked four wide, GPU LBVH, host SAH walked binary), the session forms, sample
lanes, the AETHER post, row strips and the allocator's poison patterns; the 600 000-triangle stand-in of BASELINE
configs[3] (the bottom-up pass under real concurrency); sessions that share one cached mesh; the memory a refit may and may
not take; another topology; refusals; a re-mesh enqueued behind frames without a host wait; render_terrain_mesh_sequence.
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
TREE = ("mesh_scalars", "bvh_nodes", "bvh_triangles")  # fingerprint entries of the tree itself: all that may differ
MOTIONS = ("shift", "jitter", "permuted", "collapsed", "away", "back", "combined")
SEEN = {"shift": True, "jitter": True, "permuted": True, "collapsed": False, "away": False, "back": True, "combined": True}
CAM_7 = CHAIN[3][0]


def _city():
    return scenes.box_city(n_boxes=30, seed=5)


def _steps(v):
    """The chain: (motion, vertices, camera or None, re-armable values given with it)."""
    rng = np.random.default_rng(2024)
    jitter = (v + rng.uniform(-8.0, 8.0, v.shape)).astype(np.float32)
    jitter[:, 1] = np.maximum(jitter[:, 1], 0.0)
    return [
        ("shift", (v + np.float32([6.0, 2.0, -4.0])).astype(np.float32), None, {}),
        ("jitter", jitter, None, {}),
        ("permuted", v[rng.permutation(len(v))].copy(), None, dict(seed=11)),
        ("collapsed", np.tile(v[17], (len(v), 1)).astype(np.float32), None, {}),
        ("away", (v + np.float32(1e4)).astype(np.float32), None, {}),
        ("back", v.copy(), None, {}),
        ("combined", (v + np.float32([-9.0, 3.0, 7.0])).astype(np.float32), CAM_7, dict(sun_azimuth_deg=80.0, sun_elevation_deg=20.0, max_frames=3, min_frames=3)),
    ]


def _held(cam, kw, steps):
    """(camera, render keywords) of every step: a re-mesh keeps the camera and every re-armable value it is not given."""
    held, camera, out = dict(kw), dict(cam), []
    for _, verts, new_cam, change in steps:
        held = {**held, **change, "mesh_vertices": verts}
        camera = dict(new_cam) if new_cam is not None else camera
        out.append((dict(camera), held))
    return out


def _same(got, want, what=""):
    """Bit for bit on the outputs and on every scalar but gpu_resource_bytes (the refit's own tables: checked apart)."""
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key}"
    for key in SCALARS:
        if key in want and key != "gpu_resource_bytes":
            assert got[key] == want[key], f"{what}: {key} {got[key]!r} != {want[key]!r}"


def _differs(a, b):
    return float(((a != b) & ~(np.isnan(a) & np.isnan(b))).mean())


_ORACLE = {}


def _oracle(dem, i, c, k):
    from oracle import oracle

    if i not in _ORACLE:
        _ORACLE[i] = oracle.render(dem, W, H, c, **k)
    return _ORACLE[i]


def _chain(dem, cam, kw, oneshot=True, with_oracle=False, steps=None, **opts):
    """Re-mesh one session along the chain; every step against a fresh session with the moved mesh (and the one-shot, and
    the oracle); returns the results."""
    import forge3d_amd as f3d

    steps = steps if steps is not None else _steps(kw["mesh_vertices"])
    s = _session(dem, cam, kw, **opts)
    out, bytes_seen = [], []
    try:
        for i, ((motion, verts, new_cam, change), (c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            s.remesh(verts, None, new_cam, **change)
            with _session(dem, c, k, **opts) as fresh:
                got_state, want_state = _state(s), _state(fresh)
                for key in ("gbuffer", "reservoirs", "accumulation", "frame_heads"):
                    if key in want_state[0]:
                        assert got_state[0][key] == want_state[0][key], f"step {i} ({motion}): {key}"
                assert got_state[1] == want_state[1], f"step {i} ({motion}): certificates"
                differ = sorted(key for key in want_state[0] if got_state[0][key] != want_state[0][key])
                assert set(differ) <= set(TREE), f"step {i} ({motion}): fingerprint entries {differ} differ"
                want = fresh.render()
            got = s.render()
            _same(got, want, f"step {i} ({motion}) vs a fresh session")
            assert got["gpu_resource_bytes"] >= want["gpu_resource_bytes"], (i, motion)
            bytes_seen.append((got["gpu_resource_bytes"], want["gpu_resource_bytes"]))
            if oneshot:
                _same(got, f3d.hybrid_render_terrain_reference(dem, W, H, c, **k), f"step {i} ({motion}) vs the one-shot")
                bare = {key: val for key, val in k.items() if key not in ("mesh_vertices", "mesh_indices")}
                share = _differs(got["depth"], f3d.hybrid_render_terrain_reference(dem, W, H, c, **bare)["depth"])
                print(f"step {i} ({motion}): depth differs from the mesh-less render on {share:.3f} of the pixels")
                if SEEN[motion]:
                    assert share >= 0.10, (motion, share)  # the moved mesh is in the picture
                else:
                    assert share == 0.0, (motion, share)
            if with_oracle:
                want = _oracle(dem, i, c, k)
                for key in AOVS:
                    assert np.array_equal(got[key], want[key], equal_nan=True), (i, motion, key, "oracle")
            out.append(got)
        assert len({b for b, _ in bytes_seen}) == 1, bytes_seen  # constant from the first refit on
    finally:
        s.close()
    return out


def _mesh_scene():
    dem, cam, kw = _golden()
    v, t = _city()
    return dem, cam, dict(kw, mesh_vertices=v, mesh_indices=t)


@pytest.mark.parametrize("builder", [1, 2, 3], ids=["host-bvh4", "gpu-lbvh", "host-binary"])
def test_chain_on_the_golden_dem_equals_fresh_sessions_one_shots_and_the_oracle(builder):
    dem, cam, kw = _mesh_scene()
    got = _chain(dem, cam, kw, oneshot=True, with_oracle=True, mesh_builder=builder)
    assert not np.array_equal(got[0]["rgba"], got[5]["rgba"])  # (the shift alone changes the image)


@pytest.mark.parametrize("opts", [dict(frames_in_flight=0), dict(frames_in_flight=4), dict(frames_in_flight=0, bands=3, band_streams=2)],
                         ids=["fused", "in-flight-4", "bands"])
def test_chain_across_session_forms(opts):
    dem, cam, kw = _mesh_scene()
    _chain(dem, cam, kw, oneshot=False, **opts)


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_chain_across_sample_lanes(lanes):
    from forge3d_amd.session import kernel_variant

    dem, cam, kw = _mesh_scene()
    _chain(dem, cam, dict(kw, spp=8), oneshot=False, frames_in_flight=0, kernel_variant=kernel_variant(sample_lanes=lanes))


def test_chain_with_the_aether_post():
    import forge3d_amd as f3d
    from forge3d_amd import _native

    dem, cam, kw = _mesh_scene()
    handle = _native._resolve_atmosphere({"turbidity": 3.0})
    steps = _steps(kw["mesh_vertices"])
    s = _session(dem, cam, dict(kw, atmosphere=handle))
    try:
        for i, ((motion, verts, new_cam, change), (c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            s.remesh(verts, None, new_cam, **change)
            got = s.render()
            _same(got, f3d.hybrid_render_terrain_reference(dem, W, H, c, atmosphere={"turbidity": 3.0}, **k), f"aether step {i} ({motion})")
    finally:
        s.close()
    c, k = _held(cam, kw, steps)[-1]
    assert not np.array_equal(got["rgba"], f3d.hybrid_render_terrain_reference(dem, W, H, c, **k)["rgba"])  # (the post is on)


@pytest.mark.parametrize("in_flight", [0, 4])
def test_remeshed_row_strips_equal_the_whole_image(in_flight):
    """Two strips with caller-owned reservoirs and the device-copy halo exchange (as test_gpu_reaim's strip test)."""
    import torch

    import forge3d_amd as f3d
    from forge3d_amd.session import HALO_ROWS as R, TerrainSession, reservoir_buffer_bytes

    dem, cam, kw = _mesh_scene()
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

    steps = [st for st in _steps(kw["mesh_vertices"]) if st[0] in ("shift", "permuted", "back", "combined")]
    try:
        render(4)
        for i, ((motion, verts, new_cam, change), (c, k)) in enumerate(zip(steps, _held(cam, kw, steps))):
            for s in sessions:
                s.remesh(verts, None, new_cam, **change)
            got = render(int(k["max_frames"]))
            want = f3d.hybrid_render_terrain_reference(dem, W, H, c, **k)
            for key in AOVS:
                assert np.array_equal(got[key], want[key], equal_nan=True), (i, motion, key)
    finally:
        for s in sessions:
            s.close()


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_remesh as t
dem, cam, kw = t._mesh_scene()
out = {}
for name, opts in (("wide", {"mesh_builder": 1}), ("lbvh", {"mesh_builder": 2}), ("binary", {"mesh_builder": 3, "frames_in_flight": 0})):
    s = t._session(dem, cam, kw, **opts)
    for j, (motion, verts, new_cam, change) in enumerate(t._steps(kw["mesh_vertices"])):
        s.remesh(verts, None, new_cam, **change)
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
    """What a refit reads it must have written: with the allocator filling every buffer with a pattern, a parent link, a
    counter, a bound or a box the passes forget would carry the pattern into the walk."""
    with tempfile.TemporaryDirectory() as tmp:
        plain = _chain_in_child(None, Path(tmp) / "plain.npz")
        assert len(plain) == 3 * len(MOTIONS) * len(AOVS)
        for pattern in (0, 0x5A, 0xFF):
            got = _chain_in_child(pattern, Path(tmp) / f"p{pattern}.npz")
            assert sorted(got) == sorted(plain)
            for key in plain:
                assert np.array_equal(got[key], plain[key], equal_nan=True), (pattern, key)


def test_refit_of_the_600k_triangle_standin_equals_a_fresh_session_and_the_oracle_sweep():
    """The scene of test_config4_standin_600k_triangles_matches_the_oracle_sweep (tests/test_gpu_parity.py): a tenth of the
    50 000 boxes raised by 5..30 m, then every box raised.  600 000 leaf-order triangles and ~300 000 nodes climb their
    trees at once: the test of the bottom-up pass under real concurrency.  Run once."""
    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession
    from oracle import oracle

    dem = datasets.rainier_proxy(512)
    spacing = 40.0
    v, t = datasets.proxy_buildings(dem, spacing)
    assert t.shape[0] == 600_000
    centres = v.reshape(-1, 8, 3).mean(1)
    cell = np.floor(centres[:, [0, 2]] / 250.0).astype(np.int64)
    uniq, counts = np.unique(cell, axis=0, return_counts=True)
    spot = (uniq[counts.argmax()] + 0.5) * 250.0
    near = centres[np.hypot(centres[:, 0] - spot[0], centres[:, 2] - spot[1]) < 200.0]
    target = (float(spot[0]), float(near[:, 1].mean()), float(spot[1]))
    cam = {"origin": (target[0] + 190.0, target[1] + 130.0, target[2] + 150.0), "look_at": target, "up": (0.0, 1.0, 0.0), "fov_y": 55.0,
           "exposure": 1.0}
    kw = dict(spacing=(spacing, spacing), exaggeration=1.0, albedo=(0.6, 0.6, 0.6), sun_azimuth_deg=302.0, sun_elevation_deg=24.0, spp=2,
              max_frames=2, min_frames=2, variance_threshold=1e30, mesh_vertices=v, mesh_indices=t)
    rng = np.random.default_rng(7)
    boxes = len(v) // 8
    lift = np.zeros(boxes, np.float32)
    lift[rng.permutation(boxes)[:boxes // 10]] = rng.uniform(5.0, 30.0, boxes // 10).astype(np.float32)
    tenth = v.copy()
    tenth[:, 1] += np.repeat(lift, 8)
    every = v.copy()
    every[:, 1] += np.repeat(rng.uniform(5.0, 30.0, boxes).astype(np.float32), 8)
    wants = []
    for verts in (tenth, every):
        want = oracle.render(dem, 64, 64, cam, **dict(kw, mesh_vertices=verts))
        assert float((want["albedo"][..., 2] > 0.75).mean()) > 0.05  # buildings are really in view (mesh albedo .7,.7,.8)
        wants.append(want)
    assert not np.array_equal(wants[0]["depth"], wants[1]["depth"], equal_nan=True)
    for builder in (1, 2):
        with TerrainSession(dem, 64, 64, cam, mesh_builder=builder, **kw) as s:
            for verts, want in zip((tenth, every), wants):
                s.remesh(verts)
                got = s.render()
                with TerrainSession(dem, 64, 64, cam, mesh_builder=builder, **dict(kw, mesh_vertices=verts)) as fresh:
                    _same(got, fresh.render(), f"600k triangles, builder {builder}, vs a fresh session")
                assert np.float32(got["variance"]) == np.float32(want["variance"]), builder
                for key in AOVS:
                    assert np.array_equal(got[key], want[key], equal_nan=True), (builder, key)


def test_a_remesh_leaves_the_shared_mesh_of_other_sessions_alone():
    dem, cam, kw = _mesh_scene()
    moved = _steps(kw["mesh_vertices"])[0][1]
    with _session(dem, cam, kw) as a, _session(dem, cam, kw) as b:
        before = _state(b)
        assert _state(a) == before  # one cached mesh, two sessions
        original = b.render()
        a.remesh(moved)
        got = a.render()
        assert not np.array_equal(got["depth"], original["depth"], equal_nan=True)
        b.rearm()
        after = _state(b)
        for key in ("mesh_scalars", "mesh_vertices", "mesh_indices", "bvh_nodes", "bvh_triangles"):
            assert after[0][key] == before[0][key], key
        _same(b.render(), original, "the session that shares the mesh")
        with _session(dem, cam, kw) as c:  # (the cache entry itself still holds the original mesh)
            assert _state(c)[0]["bvh_nodes"] == before[0]["bvh_nodes"] and _state(c)[0]["mesh_vertices"] == before[0]["mesh_vertices"]
            _same(c.render(), original, "a session created afterwards with the original mesh")
        with _session(dem, cam, dict(kw, mesh_vertices=moved)) as fresh:
            _same(got, fresh.render(), "the re-meshed session")


def test_ten_refits_after_the_first_take_no_memory_and_a_small_budget_refuses_the_first():
    dem, cam, kw = _golden()
    v, t = scenes.box_city(n_boxes=400, seed=5)  # (4 800 triangles: the refit's tables outweigh the slack of the create's own budget gate)
    kw = dict(kw, mesh_vertices=v, mesh_indices=t)
    opts = dict(frames_in_flight=0, mesh_builder=3)
    with _session(dem, cam, kw, **opts) as s:
        created = s.info()
        s.remesh(v + np.float32(1.0))
        tables = s.info()["gpu_resource_bytes"] - created["gpu_resource_bytes"]
        assert 2 * 4 * len(t) // 4 + 48 <= tables <= 2 * 4 * 2 * len(t) + 48  # two words a node (leaves of <= 4 triangles, < 2 nodes a triangle) + the bounds
        assert {k: val for k, val in s.info().items() if k != "gpu_resource_bytes"} == {k: val for k, val in created.items() if k != "gpu_resource_bytes"}
        s.render()
        first = s.info()
        assert first["gpu_resource_bytes"] == created["gpu_resource_bytes"] + tables
        for i in range(10):
            s.remesh(v + np.float32(0.5 * i), None, dict(ORBIT, fov_y=40.0 + i) if i % 2 else None, seed=i)
            assert s.info() == first
        s.render()
        assert s.info() == first
        need = created["gpu_resource_bytes"]
    # the smallest budget (in KiB steps) the create accepts leaves no room for the refit's tables
    for budget in range(need, need + (64 << 10), 1 << 10):
        try:
            s = _session(dem, cam, kw, memory_budget_bytes=budget, **opts)
            break
        except RuntimeError as e:
            assert "exceeds the memory budget" in str(e)
    else:
        raise AssertionError("no budget accepted")
    with s:
        assert budget < need + tables
        want = s.render()
        with pytest.raises(RuntimeError, match="re-mesh exceeds the memory budget"):
            s.remesh(v + np.float32(1.0))
        assert s.info()["gpu_resource_bytes"] == need
        s.rearm()
        _same(s.render(), want, "after a refit the budget refused")
        with _session(dem, cam, kw, **opts) as roomy:
            _same(want, roomy.render(), "the old mesh")


def test_another_topology_equals_a_fresh_session_with_its_bytes():
    import forge3d_amd as f3d

    dem, cam, kw = _mesh_scene()
    v2, t2 = scenes.box_city(n_boxes=12, seed=9)
    for builder in (1, 2):
        with _session(dem, cam, kw, mesh_builder=builder) as s:
            s.remesh(kw["mesh_vertices"] + np.float32(2.0))  # (its own copy first: the new mesh must take it back)
            s.remesh(v2, t2, ORBIT, seed=4)
            k = dict(kw, mesh_vertices=v2, mesh_indices=t2, seed=4)
            with _session(dem, ORBIT, k, mesh_builder=builder) as fresh:
                assert _state(s) == _state(fresh)
                want = fresh.render()
            got = s.render()
            _same(got, want, "another topology")
            assert got["gpu_resource_bytes"] == want["gpu_resource_bytes"]
            _same(got, f3d.hybrid_render_terrain_reference(dem, W, H, ORBIT, **k), "another topology vs the one-shot")
            s.remesh(v2 + np.float32([3.0, 0.0, 1.0]))  # and the new mesh moves like the first
            with _session(dem, ORBIT, dict(k, mesh_vertices=v2 + np.float32([3.0, 0.0, 1.0])), mesh_builder=builder) as fresh:
                _same(s.render(), fresh.render(), "the new topology refitted")
            # the same indices again: a fresh tree
            s.remesh(v2, t2)
            with _session(dem, ORBIT, k, mesh_builder=builder) as fresh:
                assert _state(s) == _state(fresh)


def test_refusals_leave_the_session_rendering_the_old_mesh():
    import forge3d_amd as f3d
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = _mesh_scene()
    v, t = kw["mesh_vertices"], kw["mesh_indices"]
    moved = (v + np.float32([6.0, 2.0, -4.0])).astype(np.float32)
    nan = moved.copy()
    nan[5, 1] = np.nan
    with _session(dem, cam, kw) as s:
        s.remesh(moved, seed=5)
        state = _state(s)
        want = s.render()
        with pytest.raises(RuntimeError, match="mesh vertices contain non-finite values"):
            s.remesh(nan)
        with pytest.raises(RuntimeError, match="mesh vertices contain non-finite values"):
            s.remesh(nan, t)
        with pytest.raises(RuntimeError) as one_shot:
            f3d.hybrid_render_terrain_reference(dem, W, H, cam, **dict(kw, mesh_vertices=nan))
        assert "mesh vertices contain non-finite values" in str(one_shot.value)
        with pytest.raises(ValueError, match=f"{len(v) - 3} vertices given, its topology has {len(v)}"):
            s.remesh(moved[:-3])
        with pytest.raises(RuntimeError, match="mesh indices reference out-of-bounds vertices"):
            s.remesh(moved[:-3], t)
        with pytest.raises(RuntimeError):  # a camera the create refuses: with the mesh untouched
            s.remesh(v, None, dict(ORBIT, look_at=ORBIT["origin"]))
        with pytest.raises(ValueError, match="re-arm it"):
            s.render()
        s.rearm()
        assert _state(s) == state
        _same(s.render(), want, "after refused re-meshes")
        _same(want, f3d.hybrid_render_terrain_reference(dem, W, H, cam, **dict(kw, mesh_vertices=moved, seed=5)), "the old mesh")
    bare = {key: val for key, val in kw.items() if key not in ("mesh_vertices", "mesh_indices")}
    with _session(dem, cam, bare) as s:
        want = s.render()
        for indices in (None, t):
            with pytest.raises(ValueError, match="created without a mesh"):
                s.remesh(v, indices)
        s.rearm()
        _same(s.render(), want, "a session without a mesh")
    bounds = [(0, 29), (29, 64)]
    sessions = [TerrainSession(dem, W, H, cam, row_begin=b, row_end=e, **kw) for b, e in bounds]
    try:
        exports = [x.halo_export() for x in sessions]
        sessions[0].halo_connect(1, exports[1])
        sessions[1].halo_connect(0, exports[0])
        for x in sessions:
            with pytest.raises(ValueError, match="a session with peer halos cannot be re-meshed"):  # (status 1)
                x.remesh(moved)
    finally:
        for x in sessions:
            x.close()


def test_remesh_without_a_host_wait_after_frames_and_a_device_resolve_and_after_a_pool_trim():
    import torch

    from forge3d_amd import _native

    dem, cam, kw = _mesh_scene()
    dev = torch.device("cuda", 0)
    steps = [st for st in _steps(kw["mesh_vertices"]) if st[0] in ("shift", "jitter", "back")]  # (they keep the 4-frame budget)
    held = _held(cam, kw, steps)
    rgba = [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(len(steps) + 1)]
    with _session(dem, cam, kw, frames_in_flight=0) as s:
        for i in range(len(steps) + 1):
            if i:
                s.remesh(steps[i - 1][1], None, steps[i - 1][2], **steps[i - 1][3])  # (behind the frames and the resolve just enqueued)
            s.enqueue_frames(0, 4)
            s.resolve_device(4, d_rgba=rgba[i].data_ptr())
        torch.cuda.synchronize()
        for i, (c, k) in enumerate([(cam, kw)] + held):
            with _session(dem, c, k, frames_in_flight=0) as fresh:
                assert np.array_equal(rgba[i].cpu().numpy(), fresh.render()["rgba"]), i
        _native.lib().f3d_device_pool_trim()
        s.remesh(steps[1][1])
        with _session(dem, *held[1], frames_in_flight=0) as fresh:
            _same(s.render(), fresh.render(), "after a trim")


def test_render_terrain_mesh_sequence_equals_one_shots():
    import forge3d_amd as f3d
    from forge3d_amd.path_tracing import render_terrain_mesh_sequence

    dem, cam, kw = _mesh_scene()
    v, t = kw["mesh_vertices"], kw["mesh_indices"]
    v2, t2 = scenes.box_city(n_boxes=12, seed=9)
    common = {key: val for key, val in kw.items() if key not in ("sun_azimuth_deg", "sun_elevation_deg")}
    sun = dict(sun_azimuth_deg=225.0, sun_elevation_deg=35.0)
    frames = [dict(sun), dict(sun, mesh_vertices=v + np.float32([6.0, 2.0, -4.0])),
              dict(sun, mesh_vertices=v + np.float32([12.0, 4.0, -8.0]), camera=ORBIT),
              dict(camera=ORBIT, sun_azimuth_deg=10.0, sun_elevation_deg=12.0, seed=99, max_frames=3, min_frames=3),   # no mesh key: common's again
              dict(sun, mesh_vertices=v2, mesh_indices=t2),                                                              # another mesh
              dict(sun, mesh_vertices=v2 + np.float32([0.0, 5.0, 0.0]), mesh_indices=t2, sun_color=(0.5, 0.6, 1.0)),     # ... moved: a refit
              dict(sun, mesh_vertices=v + np.float32([1.0, 0.0, 1.0]))]                                                   # common's indices again
    got = list(render_terrain_mesh_sequence(dem, W, H, cam, frames=frames, **common))
    assert len(got) == len(frames)
    for i, frame in enumerate(frames):  # item i is the one-shot with **common, **frames[i]: a key a frame does not name is common's
        rest = {k: val for k, val in frame.items() if k != "camera"}
        want = f3d.hybrid_render_terrain_reference(dem, W, H, frame.get("camera", cam), **{**common, **rest})
        assert sorted(got[i]) == sorted(want)
        _same(got[i], want, f"sequence frame {i}")
    assert not np.array_equal(got[0]["depth"], got[1]["depth"], equal_nan=True)
