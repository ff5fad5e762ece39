"""`-m gpu`: ray queries on a live terrain session (f3d_session_query: pick, line of sight, ground).

The device against the oracle and against the kernel's own lane body run on the host (tests/query_host), bit for bit: the
proof rays (closest hit; occlusion with and without the curvature policy), the ground rays, the pixel query over a whole view
of the box city for the three tree builders and for a row strip that answers every row, batch sizes around the wave size.
The query follows the live scene with no host wait between the update and the query (re-aim, re-mesh, re-terrain), reads and
never writes what the frames read (fingerprint, renders with queries interleaved), takes device tensors without a copy or
an allocation, keeps its host scratch between calls, and its refusals leave the session rendering what it rendered.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from oracle import oracle
from test_gpu_reaim import AUTO, H, ORBIT, W, _same
from test_session_query_host import (NONE, QNAN, HostScene, _bits, _ground_points, _kw, _oracle_batch, _rays_of, bad_ray_set,
                                     harness)  # noqa: F401  (harness: the host body's fixture)

pytestmark = pytest.mark.gpu

KEYS = ("kind", "t", "normal", "position", "primitive")


def _equal(got, want, keys=KEYS, what=""):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype == np.float32:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), f"{what}: {k}"


def _city():
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    return dem, verts, tris, _kw(dem, mesh_vertices=verts, mesh_indices=tris)


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or scenes.CAM), **opts, **kw)


PIXELS = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.uint32)


@pytest.fixture(scope="module")
def city_host(harness):  # noqa: F811
    """The host body's answers for the city: the pixel query over the whole view (computed once, shared, never written)."""
    dem, verts, tris, kw = _city()
    scene = HostScene(harness, dem, scenes.CAM, kw)
    picked = scene.run(2, PIXELS)
    for v in picked.values():
        v.setflags(write=False)
    yield scene, picked
    scene.close()


def test_the_library_exports_the_query():
    from forge3d_amd import _native
    from forge3d_amd.session import TerrainSession

    assert _native.lib().f3d_session_query is not None and _native.lib().f3d_abi_version() == 6
    assert callable(TerrainSession.trace) and callable(TerrainSession.pick)


# ---- 1. device against oracle and host body ---------------------------------------------------------------------------------
def test_proof_rays_equal_the_oracle(harness):  # noqa: F811
    heights, rays = scenes.proof_rays(n_random=2000, mask=False)
    kw = dict(_kw(heights), spacing=(500.0, 500.0), exaggeration=1.0)
    cam = {"origin": (0.0, 9000.0, 90000.0), "look_at": (0.0, 900.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}
    ox = np.float32(-0.5 * 255.0 * 500.0)
    rays = rays.copy()
    rays[:, 0] += ox
    rays[:, 2] += ox
    host = HostScene(harness, heights, cam, kw)  # (the curvature constants of this scene: the same fill_uniforms)
    try:
        assert host.origin == (ox, ox)
        with _session(heights, kw, cam) as s:
            got = s.trace(rays)
            want = _oracle_batch(host, heights, rays, 500.0, 1.0, any_hit=False, apply_curvature=False)
            hit = want["hit"] != 0
            assert np.array_equal(got["kind"], hit.astype(np.uint32))
            assert np.array_equal(_bits(got["t"])[hit], _bits(want["t"])[hit]) and np.all(_bits(got["t"])[~hit] == QNAN)
            assert np.array_equal(_bits(got["normal"])[hit], _bits(want["normal"])[hit])
            for curved in (False, True):
                occ = s.occluded(rays, curved=curved)
                want = _oracle_batch(host, heights, rays, 500.0, 1.0, any_hit=True, apply_curvature=curved)
                assert occ.dtype == bool and np.array_equal(occ, want["hit"] != 0), f"curved={curved}"
    finally:
        host.close()


def test_ground_equals_the_oracle(city_host):
    host, _ = city_host
    dem, _, _, kw = _city()
    spacing = kw["spacing"][0]
    xz, n_inner = _ground_points(dem, spacing)
    top = np.float32(float(dem.max()) * kw["exaggeration"] + 10.0)
    rays = np.zeros((len(xz), 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5], rays[:, 7] = xz[:, 0], top, xz[:, 1], -1.0, 1e30
    want = _oracle_batch(host, dem, rays, spacing, kw["exaggeration"], any_hit=False, apply_curvature=False)
    hit = want["hit"] != 0
    with _session(dem, kw) as s:
        y = s.ground(xz)  # (terrain only: the city does not count as ground)
    assert y.dtype == np.float32 and np.array_equal(np.isnan(y), ~hit) and hit[:n_inner].all()
    assert np.array_equal(_bits(y)[hit], _bits(top - want["t"])[hit])


@pytest.mark.parametrize("mesh_builder", [0, 2, 3])
def test_pick_equals_the_host_body(city_host, mesh_builder):
    _, want = city_host
    dem, _, _, kw = _city()
    with _session(dem, kw, mesh_builder=mesh_builder) as s:
        got = s.pick(PIXELS)
        _equal(got, want, KEYS + ("direction",), f"builder {mesh_builder}")
        again = s.trace(_rays_of(got))
        _equal(again, want, KEYS, "mode 0 fed mode 2's directions")


def test_pick_equals_the_oracles_aovs(city_host):
    _, want = city_host
    dem, _, _, kw = _city()
    ref = oracle.render(dem, W, H, scenes.CAM, **kw)
    with _session(dem, kw) as s:
        got = s.pick(PIXELS)
    assert np.array_equal(_bits(got["t"]), _bits(ref["depth"]).reshape(-1))
    half = got["normal"].astype(np.float16).astype(np.float32)  # the normal AOV goes through RGBA16F
    assert np.array_equal(_bits(half), _bits(ref["normal"]).reshape(-1, 3))
    mesh_albedo = _bits(np.array([0.7, 0.7, 0.8], np.float32).astype(np.float16).astype(np.float32))
    assert np.array_equal(got["kind"] == 2, np.all(_bits(ref["albedo"]).reshape(-1, 3) == mesh_albedo, axis=1))


def test_a_strip_session_answers_every_row_and_batch_sizes(city_host):
    _, want = city_host
    dem, _, _, kw = _city()
    with _session(dem, kw, row_begin=16, row_end=40) as s:
        _equal(s.pick(PIXELS), want, KEYS + ("direction",), "strip session, all rows")
        for n in (1, 63, 64, 65):
            _equal(s.pick(PIXELS[-n:]), {k: v[-n:] for k, v in want.items()}, KEYS + ("direction",), f"count {n}")
        empty = s.pick(PIXELS[:0])
        assert all(len(v) == 0 for v in empty.values())


# ---- 2. the query follows the live scene ------------------------------------------------------------------------------------
def test_pick_follows_a_reaim_without_a_wait():
    dem, _, _, kw = _city()
    with _session(dem, kw) as s, _session(dem, kw, ORBIT) as fresh:
        before = s.pick(PIXELS)
        s.reaim(ORBIT)
        got = s.pick(PIXELS)  # (nothing between the update and the query)
        want = fresh.pick(PIXELS)
        _equal(got, want, KEYS + ("direction",), "after reaim")
        assert not np.array_equal(before["kind"], got["kind"])


@pytest.mark.parametrize("mesh_builder", [0, 2])
def test_trace_follows_a_remesh_without_a_wait(city_host, mesh_builder):
    _, picked = city_host
    dem, verts, tris, kw = _city()
    shift = np.array([6.0, 2.0, -4.0], np.float32)
    rays = _rays_of(picked)
    moved = rays.copy()
    moved[:, 0:3] += shift  # the rays move with the mesh: what they hit of it stays
    with _session(dem, kw, mesh_builder=mesh_builder) as s:
        before = s.trace(rays)
        s.remesh(verts + shift)
        got = s.trace(moved)
        same_rays = s.trace(rays)
    with _session(dem, dict(kw, mesh_vertices=verts + shift), mesh_builder=mesh_builder) as fresh:
        _equal(got, fresh.trace(moved), KEYS, "after remesh (refitted tree) vs a fresh session")
        _equal(same_rays, fresh.trace(rays), KEYS, "after remesh, the old rays")
    assert not np.array_equal(before["kind"], same_rays["kind"])
    still = (before["kind"] == 2) & (got["kind"] == 2) & (before["primitive"] // 12 == got["primitive"] // 12)  # 12 triangles a box
    assert still.sum() > 1000 and np.array_equal(before["primitive"][still], got["primitive"][still])


def test_ground_follows_a_reterrain_without_a_wait(city_host):
    host, _ = city_host
    dem, _, _, kw = _city()
    spacing = kw["spacing"][0]
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(np.float32)  # raised: still under top
    result = dem.copy()
    result[20:36, 20:36] = patch
    ox, oz = float(host.origin[0]), float(host.origin[1])
    xz = np.stack([rng.uniform(ox + 20 * spacing, ox + 35 * spacing, 500), rng.uniform(oz + 20 * spacing, oz + 35 * spacing, 500)], 1).astype(np.float32)
    top = np.float32(float(result.max()) * kw["exaggeration"] + 10.0)
    with _session(dem, kw) as s:
        before = s.ground(xz, top=top)
        s.reterrain(patch, at=(20, 20))
        got = s.ground(xz, top=top)
    rays = np.zeros((len(xz), 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5], rays[:, 7] = xz[:, 0], top, xz[:, 1], -1.0, 1e30
    want = _oracle_batch(host, result, rays, spacing, kw["exaggeration"], any_hit=False, apply_curvature=False)
    assert (want["hit"] != 0).all() and np.array_equal(_bits(got), _bits(top - want["t"]))
    assert np.all(got > before), "the patch raised the ground under every point"


# ---- 3. read-only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames_in_flight", [0, AUTO])
def test_queries_change_nothing_a_frame_reads(city_host, frames_in_flight):
    _, picked = city_host
    dem, _, _, kw = _city()
    rays = _rays_of(picked)
    with _session(dem, kw, frames_in_flight=frames_in_flight) as s, _session(dem, kw, frames_in_flight=frames_in_flight) as plain:
        fp = s.fingerprint()
        s.pick(PIXELS), s.trace(rays), s.occluded(rays), s.ground(rays[:, 0:2])
        assert s.fingerprint() == fp
        n = 4
        for f in range(n):
            s.enqueue_frames(f, 1, f + 1 == n)
            s.pick(PIXELS[: 65 + f])
            s.occluded(rays[:100], curved=True)
            plain.enqueue_frames(f, 1, f + 1 == n)
        got, want = s.resolve(n), plain.resolve(n)
        for k in ("rgba", "albedo", "normal", "depth"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.window_stats() == plain.window_stats()


# ---- 4. device pointers -----------------------------------------------------------------------------------------------------
def test_tensor_queries_copy_and_allocate_nothing(city_host):
    import torch

    _, want = city_host
    dem, _, _, kw = _city()
    rays = _rays_of(want)
    with _session(dem, kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        d_pixels = torch.from_numpy(PIXELS.astype(np.int32)).cuda()
        d_rays = torch.from_numpy(rays).cuda()
        got = s.pick(d_pixels)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
        host = {k: v.cpu().numpy().view(np.uint32 if k in ("kind", "primitive") else np.float32) for k, v in got.items()}
        _equal(host, want, KEYS + ("direction",), "tensor pick")
        later = s.trace(d_rays, wait=False)  # NO_WAIT: in flight on the session's stream (the null stream here)
        torch.cuda.current_stream().synchronize()
        _equal({k: v.cpu().numpy().view(np.uint32 if k in ("kind", "primitive") else np.float32) for k, v in later.items()}, want, KEYS,
               "tensor trace, no wait")
        occ = s.occluded(d_rays)
        y = s.ground(d_rays[:, 0:2].contiguous())
        assert s.info()["gpu_resource_bytes"] == bytes0, "the device form takes nothing"
        assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), s.occluded(rays))
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(s.ground(rays[:, 0:2])))
        # the device form took nothing; the host form (used just above) took its scratch once
        grown = s.info()["gpu_resource_bytes"]
        assert grown == bytes0 + 80 * len(rays)
        s.pick(d_pixels), s.trace(d_rays)
        s.pick(PIXELS[:100]), s.trace(rays)
        assert s.info()["gpu_resource_bytes"] == grown, "a smaller or equal batch reuses the scratch"
        s.trace(np.concatenate([rays, rays[:7]]))
        assert s.info()["gpu_resource_bytes"] == bytes0 + 80 * (len(rays) + 7), "a larger batch grows it, the old one goes back"


def test_a_batch_larger_than_the_staging_buffers(city_host):
    """405 504 rays: 12.4 MiB up and up to 4.6 MiB per output down, each through the two 4 MiB pinned staging buffers more
    than once (the size at which the staged copies take their chunked path)."""
    import torch

    _, want = city_host
    dem, _, _, kw = _city()
    rays = np.tile(_rays_of(want), (66, 1))
    with _session(dem, kw) as s:
        got = s.trace(rays)
        _equal(got, {k: np.tile(want[k], (66,) + (1,) * (want[k].ndim - 1)) for k in KEYS}, KEYS, "host form, chunked copies")
        dev = s.trace(torch.from_numpy(rays).cuda())
        _equal({k: v.cpu().numpy().view(np.uint32 if k in ("kind", "primitive") else np.float32) for k, v in dev.items()}, got, KEYS,
               "device form")
        assert np.array_equal(s.occluded(rays), np.tile(s.occluded(rays[:6144]), 66))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def _raw(s, rays, mode=0, flags=0, struct_size=None, **outputs):
    from forge3d_amd import _native

    q = _native.QueryDesc()
    q.struct_size = C.sizeof(_native.QueryDesc) if struct_size is None else struct_size
    q.mode, q.flags, q.count, q.rays = mode, flags, len(rays), rays.ctypes.data
    for k, v in outputs.items():
        setattr(q, k, v.ctypes.data)
    s._check(s._lib.f3d_session_query(s._handle, C.byref(q), s._err, len(s._err)))


def test_refusals_leave_the_session_rendering_what_it_rendered(city_host):
    _, picked = city_host
    dem, _, _, kw = _city()
    kw = scenes.fixed_frames(kw, 4)
    rays = np.ascontiguousarray(_rays_of(picked)[:1024])
    kind, t = np.zeros(1024, np.uint32), np.zeros(1024, np.float32)
    with _session(dem, kw) as probe:
        need = probe.info()["gpu_resource_bytes"] + 80 * 1024
        want = probe.render()
    with _session(dem, kw, memory_budget_bytes=need - 1) as s:
        fp = s.fingerprint()
        with pytest.raises(ValueError, match="struct_size"):
            _raw(s, rays, struct_size=C.sizeof(C.c_uint32) * 4, kind=kind)
        with pytest.raises(ValueError, match="mode 1"):
            _raw(s, rays, mode=1, kind=kind, t=t)
        with pytest.raises(ValueError, match="outside the 96x64 image"):
            s.pick(np.array([[3, 5], [96, 5]], np.uint32))
        with pytest.raises(ValueError, match="outside the 96x64 image"):
            s.pick(np.array([[3, 64]], np.uint32))
        with pytest.raises(ValueError, match="NO_WAIT"):
            _raw(s, rays, flags=8, kind=kind)
        with pytest.raises(RuntimeError, match="memory budget"):
            s.trace(rays)
        assert s.info()["gpu_resource_bytes"] == need - 80 * 1024 and s.fingerprint() == fp
        assert s.trace(rays[:1023])["kind"].shape == (1023,), "one ray fewer fits"
        _same(s.render(), {k: v for k, v in want.items() if k != "gpu_resource_bytes"}, "after the refusals")
    with _session(dem, kw, memory_budget_bytes=need) as s:
        _equal(s.trace(rays), {k: v[:1024] for k, v in picked.items()}, KEYS, "the budget that fits")


# ---- 6. bad rays ------------------------------------------------------------------------------------------------------------
def test_bad_rays_answer_as_a_miss(city_host):
    host, picked = city_host
    good = _rays_of(picked)[::16]
    rays, is_bad = bad_ray_set(good)
    # the host body first, on this very set: a miss for the bad ones, no march entered
    body = host.run(0, rays)
    assert not body["kind"][is_bad].any() and not body["marches"][is_bad].any() and (body["marches"][~is_bad] == 1).all()
    dem, _, _, kw = _city()
    with _session(dem, kw) as s:
        got = s.trace(rays)
        _equal(got, body, KEYS, "device vs host body")
        assert not got["kind"][is_bad].any() and np.all(_bits(got["t"])[is_bad] == QNAN) and np.all(got["primitive"][is_bad] == NONE)
        _equal({k: v[~is_bad] for k, v in got.items()}, s.trace(good), KEYS, "the good rays answer unchanged")
        for curved in (False, True):
            occ = s.occluded(rays, curved=curved)
            assert not occ[is_bad].any() and np.array_equal(occ, host.run(1, rays, flags=2 if curved else 0)["kind"] != 0)
