"""`-m gpu`: the leaf shortcut (csrc/f3d_trace.h leaf_shortcut) on the device, bit for bit against the oracle: ray batches
through the any-hit and closest-hit march on the DEMs with the most twisted patches, ordered so that single waves hold leaves
settled by each of the three tests next to leaves that take the full path; and renders through the fused kernel with 4 and 8
sample lanes and through the frames-in-flight pipeline, whose sun and IBL rays consume the verdict alone (clear crossings)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import scenes
from leaf_scenes import checker_scene, checkerboard as _checkerboard, far_scene

pytestmark = pytest.mark.gpu

N = 64
FRAMES = 6


def checkerboard(relief=1.0):
    return _checkerboard(N, relief)


def single_saddle(relief=3.0):
    dem = np.zeros((N, N), np.float32)
    dem[31, 31] = dem[32, 32] = relief  # one twisted cell (and the ramps around it) in a plain
    dem[31, 32] = dem[32, 31] = -relief
    return dem


DEMS = {"checkerboard": checkerboard, "single saddle": single_saddle}


def _unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def ray_set(dem, seed=3):
    """Rays of every kind the shortcut tells apart, interleaved so that neighbouring lanes of a wave hold different kinds."""
    rng = np.random.default_rng(seed)
    half = 0.5 * (N - 1)
    top = float(dem.max())
    n = 1024
    kinds = []

    def rays(o, d, tmin=1e-3, tmax=1e30):
        o, d = np.asarray(o, np.float64), _unit(d)
        r = np.zeros((o.shape[0], 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
        return r

    cell = rng.integers(1, N - 2, (n, 2))
    frac = rng.random((n, 2))
    xz = cell + frac - half

    def ground(c, f):  # the bilinear patch's height
        h00, h10, h01, h11 = dem[c[:, 1], c[:, 0]], dem[c[:, 1], c[:, 0] + 1], dem[c[:, 1] + 1, c[:, 0]], dem[c[:, 1] + 1, c[:, 0] + 1]
        return (h00 * (1 - f[:, 0]) + h10 * f[:, 0]) * (1 - f[:, 1]) + (h01 * (1 - f[:, 0]) + h11 * f[:, 0]) * f[:, 1]

    y = ground(cell, frac)
    # high, flat rays over everything: clear misses with all three clearances positive (A)
    kinds.append(rays(np.c_[xz[:, 0], top + 0.3 + 2.0 * rng.random(n), xz[:, 1]], np.c_[rng.normal(size=n), 0.02 * rng.normal(size=n), rng.normal(size=n)]))
    # secondary rays: a millimetre above the patch, leaving upwards -- they start at tmin inside their cell (B)
    kinds.append(rays(np.c_[xz[:, 0], y + 1e-3, xz[:, 1]], np.c_[rng.normal(size=n), 0.3 + rng.random(n), rng.normal(size=n)]))
    # ... and leaving downwards or level: crossings in the first cells
    kinds.append(rays(np.c_[xz[:, 0], y + 1e-3 + 0.2 * rng.random(n), xz[:, 1]], np.c_[rng.normal(size=n), -0.3 * rng.random(n), rng.normal(size=n)]))
    # steep rays from above: clear crossings
    kinds.append(rays(np.c_[xz[:, 0], top + 5.0 + rng.random(n), xz[:, 1]], np.c_[0.3 * rng.normal(size=n), -1.0 - rng.random(n), 0.3 * rng.normal(size=n)]))
    # tangent rays: along a cell's diagonal the checkerboard's patch is the parabola 2 s (1 - s) relief -- level rays at its
    # apex height, a few ulp above and below (disc ~ 0); these are 45-degree lattice rays too (TIE entries)
    lat = rng.integers(2, N - 3, (n, 2))
    apex = np.float32(0.5 * top) * (1.0 + np.float32(1.1920929e-7) * rng.integers(-4, 5, n).astype(np.float32))
    sign = rng.choice([-1.0, 1.0], (n, 2))
    kinds.append(rays(np.c_[lat[:, 0] - half, apex, lat[:, 1] - half], np.c_[sign[:, 0], np.zeros(n), sign[:, 1]]))
    # 45-degree lattice rays that climb or descend slowly through the corners
    kinds.append(rays(np.c_[lat[:, 0] - half, dem[lat[:, 1], lat[:, 0]] + 0.05 + top * rng.random(n), lat[:, 1] - half],
                      np.c_[sign[:, 0], 0.08 * rng.normal(size=n), sign[:, 1]]))
    # rays along a lattice row, less than an ulp (to a few) above the highest corners they pass: they enter cells just above them
    row = rng.integers(1, N - 2, n)
    skim = np.float32(top) * (1.0 + np.float32(1.1920929e-7) * rng.integers(0, 4, n).astype(np.float32))
    kinds.append(rays(np.c_[np.full(n, -half + 0.25), skim, row - half], np.c_[np.ones(n), np.zeros(n), np.zeros(n)]))
    out = np.stack(kinds, 1).reshape(-1, 8)  # lane i holds kind i % 7
    return np.ascontiguousarray(out, np.float32)


def device_trace(dem, rays, mode, base):
    from forge3d_amd import _native

    n = rays.shape[0]
    hit, t, nrm = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    err = C.create_string_buffer(256)
    dem = np.ascontiguousarray(dem, np.float32)
    rc = _native.lib().f3d_terrain_trace_batch(dem.ctypes.data, dem.shape[1], dem.shape[0], base["origin"][0], base["origin"][1],
                                               base["spacing"][0], base["spacing"][1], 1.0, base["inv_two_r_prime"],
                                               1 if base["curvature_enabled"] else 0, rays.ctypes.data, n, int(mode),
                                               1 if base["apply_curvature"] else 0, hit.ctypes.data, t.ctypes.data, nrm.ctypes.data,
                                               err, len(err))
    assert rc == 0, err.value
    return {"hit": hit, "t": t, "normal": nrm}


@functools.lru_cache(maxsize=None)
def _ray_case(name, curved):
    """The rays and the oracle's answers, once per case and never modified.  The last eighth of the batch repeats crossing rays
    with tmax a hair beyond and a hair before the oracle's hit."""
    from oracle import oracle

    dem = DEMS[name]()
    half = 0.5 * (N - 1)
    base = dict(origin=(-half, -half), spacing=(1.0, 1.0), inv_two_r_prime=float(np.float32(1e-4)) if curved else 0.0,
                curvature_enabled=curved, apply_curvature=curved)
    rays = ray_set(dem)
    first = oracle.terrain_trace_batch(dem, rays, any_hit=False, **base)
    hits = np.flatnonzero(first["hit"])[:1024]
    near = rays[hits].copy()
    near[:, 7] = first["t"][hits] * np.where(np.arange(hits.size) & 1, np.float32(1.000001), np.float32(0.999999))
    rays = np.ascontiguousarray(np.concatenate([rays, near]), np.float32)
    want_any = oracle.terrain_trace_batch(dem, rays, any_hit=True, **base)
    want_closest = oracle.terrain_trace_batch(dem, rays, any_hit=False, **base)
    return dem, base, rays, want_any, want_closest


# the march: 2 any hit, 3 closest hit, +4 = start in the origin's cell; bits 8..15 = the ray-sharing threshold
@pytest.mark.parametrize("mode", [2, 6, 3, 7, 2 | (64 << 8), 6 | (64 << 8)])
@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("name", list(DEMS))
def test_mixed_waves_of_settled_and_full_path_leaves_match_the_oracle(name, curved, mode):
    dem, base, rays, want_any, want_closest = _ray_case(name, curved)
    assert 0.1 < want_any["hit"].mean() < 0.9, want_any["hit"].mean()
    got = device_trace(dem, rays, mode, base)
    if (mode & 3) == 3:
        assert np.array_equal(got["hit"], want_closest["hit"])
        assert np.array_equal(got["t"], want_closest["t"])
        assert np.array_equal(got["normal"], want_closest["normal"])
    else:
        bad = np.flatnonzero(got["hit"] != want_any["hit"])
        assert bad.size == 0, (bad.size, bad[:4].tolist(), rays[bad[:2]].tolist())


RENDERS = {"checkerboard x 37, sun at 5 degrees": checker_scene, "1 000 m spacing, curvature on": far_scene}


@functools.lru_cache(maxsize=None)
def _want(name):
    from oracle import oracle

    dem, cam, kw = RENDERS[name]()
    return oracle.render(dem, 64, 48, cam, **scenes.fixed_frames(kw, FRAMES, spp=8))


@pytest.mark.parametrize("opts", [dict(kernel_variant=4000000, frames_in_flight=0), dict(kernel_variant=8000000, frames_in_flight=0),
                                  dict(frames_in_flight=4)], ids=["fused S=4", "fused S=8", "in flight"])
@pytest.mark.parametrize("name", list(RENDERS))
def test_renders_are_the_oracles_bits(name, opts):
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = RENDERS[name]()
    want = _want(name)
    assert np.isfinite(want["depth"]).mean() > 0.3  # terrain fills a good part of the image
    with TerrainSession(dem, 64, 48, cam, **opts, **scenes.fixed_frames(kw, FRAMES, spp=8)) as s:
        s.enqueue_frames(0, FRAMES, True)
        m2, bad = s.window_stats()
        got = s.resolve(FRAMES)
    assert not bad
    assert np.float32(max(0.0, m2) / np.float32(FRAMES - 1)) == np.float32(want["variance"])
    for key in ("rgba", "albedo", "normal", "depth"):
        assert np.array_equal(got[key], want[key], equal_nan=True), (name, opts, key)
