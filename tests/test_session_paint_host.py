"""Vector features painted onto the drape of a live session (f3d_session_paint), the parts that need no GPU.

The lane bodies of csrc/f3d_paint.h compiled for the host (tests/paint_host) against tests/paint_reference.py, an independent
float64 statement of the contract with no tiles:

* triangle decisions equal the reference's wherever the float64 distance to the nearest edge exceeds TRIANGLE_BAND, and at most
  0.5 % of a case's texels lie inside the band; stroke coverage and blended values within COVERAGE_TOL / BLEND_TOL
  (paint_reference.py writes down where they come from);
* a triangle mesh -- jittered, and snapped to texel centres -- painted as many features at opacity 0.5 over a constant gives every
  interior texel exactly the once-blended value; a zig-zag strip that is one feature has no darker joints; the later feature
  wins; zero-area triangles, a == b, primitives off the canvas, untouched texels;
* the binning function lists, for every primitive of every case, every tile with a covered texel, and the device's walk (a
  tile's list only) returns paint_texel's bits;
* the same for primitives that cross the canvas from vertices out at the contract's reach, 2^16 texels from the terrain's centre;
* the wrapper's argument checks, the facade's validation against the recorded answers of the reference, strip expansion, the
  (z_order, id) order, header / ctypes / descriptor layout.

`host_paint` and `CASES` are what tests/test_gpu_paint.py compares the device with.
"""
from __future__ import annotations

import ctypes as C
import json
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import paint_reference as ref
from emul import emul
from test_session_drape_host import contract_pack, registration, unpack
from test_session_reterrain_host import _bare_session

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "paint_host" / "paint_harness.cpp"
f32 = np.float32
POINTS, LINES, TRIANGLES = 0, 1, 2
KINDS = {"points": POINTS, "lines": LINES, "triangles": TRIANGLES}
PRIM = np.dtype([("v", f32, 6), ("c", f32, 12), ("feature", np.uint32), ("reserved", np.uint32)])


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "paint_host")
    lib.paint_ramp_run.restype = C.c_float
    lib.paint_ramp_run.argtypes = [C.c_void_p]
    lib.paint_centres_run.restype = None
    lib.paint_centres_run.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.paint_run.restype = None
    lib.paint_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                              C.c_void_p, C.c_void_p]
    lib.paint_cov_run.restype = None
    lib.paint_cov_run.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    lib.paint_bin_run.restype = C.c_uint64
    lib.paint_bin_run.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.paint_desc_layout.restype = C.c_uint32
    lib.paint_desc_layout.argtypes = [C.c_void_p, C.c_uint32]
    return lib


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def frame_of(dem_shape, spacing, reg):
    """(origin_x, origin_z, spacing_x, spacing_z, scale_x, offset_x, scale_z, offset_z) as a session holds them, f32."""
    dem_h, dem_w = dem_shape
    sx, sz = f32(spacing[0]), f32(spacing[1])
    return np.array([f32(-0.5) * f32(dem_w - 1) * sx, f32(-0.5) * f32(dem_h - 1) * sz, sx, sz, *reg], f32)


def flipped(dem_shape, canvas):
    """A registration of the caller's: row 0 of the canvas on the DEM's LAST row (scale_z < 0)."""
    rows, cols = canvas
    return (f32(cols / (dem_shape[1] - 1)), f32(-0.5), f32(-rows / (dem_shape[0] - 1)), f32(rows - 0.5))


def scene_frame(dem_shape, spacing, canvas, kind):
    reg = flipped(dem_shape, canvas) if kind == "flipped" else registration(dem_shape, canvas, kind)
    return frame_of(dem_shape, spacing, reg)


SQUARE, ANISO = ((33, 33), (10.0, 10.0)), ((33, 17), (10.0, 7.0))  # (DEM rows x cols, spacing x / z)
# (name, DEM, canvas rows x cols, registration): the two scenes the tolerances are measured on
SCENES = [("square-70x130-area", SQUARE, (70, 130), "area"), ("aniso-257x64-flipped", ANISO, (257, 64), "flipped")]


def records(xz, rgba, indices, kind, features=None):
    """The primitive records f3d_session_paint builds: vertices gathered through the indices, the feature runs numbered."""
    xz, rgba = np.asarray(xz, f32).reshape(-1, 2), np.asarray(rgba, f32)
    if rgba.ndim == 1:
        rgba = np.broadcast_to(rgba, (len(xz), 4))
    per = kind + 1
    prims = np.asarray(indices, np.int64).reshape(-1, per)
    out = np.zeros(len(prims), PRIM)
    for k in range(3):
        v = prims[:, min(k, per - 1)]
        out["v"][:, 2 * k:2 * k + 2] = xz[v]
        out["c"][:, 4 * k:4 * k + 4] = rgba[v]
    out["feature"] = ref.feature_runs(np.asarray(features)[prims[:, 0]]) if features is not None else 0
    return out


def host_paint(lib, texels, frame, recs, kind, half_width, opacity, tiled=0, values=False):
    """One call on the host: (rows, cols) uint64 packed texels -> the same after the call (and, values=True, the f32 RGB before
    packing)."""
    texels = np.ascontiguousarray(texels, np.uint64)
    frame, recs = np.ascontiguousarray(frame, f32), np.ascontiguousarray(recs)
    out = np.zeros_like(texels)
    vals = np.zeros((*texels.shape, 3), f32) if values else None
    lib.paint_run(texels.ctypes.data, texels.shape[0], texels.shape[1], frame.ctypes.data, recs.ctypes.data, len(recs), kind, half_width, opacity,
                  tiled, out.ctypes.data, vals.ctypes.data if values else None)
    return (out, vals) if values else out


def host_cov(lib, shape, frame, rec, kind, half_width):
    frame = np.ascontiguousarray(frame, f32)
    cov, par = np.zeros(shape, f32), np.zeros((*shape, 2), f32)
    one = np.ascontiguousarray(rec).reshape(1)
    lib.paint_cov_run(shape[0], shape[1], frame.ctypes.data, one.ctypes.data, kind, half_width, cov.ctypes.data, par.ctypes.data)
    return cov, par


def host_bins(lib, shape, frame, recs, kind, half_width):
    """Per primitive the sorted list of tiles paint_bin lists."""
    frame, recs = np.ascontiguousarray(frame, f32), np.ascontiguousarray(recs)
    counts = np.zeros(len(recs), np.uint32)
    tiles = np.zeros(1 << 22, np.uint32)
    total = lib.paint_bin_run(shape[0], shape[1], frame.ctypes.data, recs.ctypes.data, len(recs), kind, half_width, counts.ctypes.data,
                              tiles.ctypes.data, len(tiles))
    assert total <= len(tiles) and int(counts.sum()) == total
    return np.split(tiles[:total], np.cumsum(counts)[:-1])


def random_canvas(shape, seed):
    return contract_pack(np.random.default_rng(seed).uniform(0.05, 0.95, (*shape, 3)).astype(f32))


def extent(frame, shape):
    """World (x_lo, x_hi, z_lo, z_hi) of the canvas's texel centres."""
    x, z = ref.centres(shape[0], shape[1], frame)
    return float(x.min()), float(x.max()), float(z.min()), float(z.max())


def case_content(kind, shape, frame, seed):
    """What one canvas is painted with, per primitive kind: (xz, rgba, indices, features, width): primitives across tile edges,
    several features, and -- over the canvas's first tile -- more primitives than two LDS chunks (2 x 64) hold."""
    rng = np.random.default_rng(seed)
    x0, x1, z0, z1 = extent(frame, shape)
    one = ref.ramp(frame)
    span = max(x1 - x0, z1 - z0, one)
    n_free, n_stack = 40, 140
    per = KINDS[kind] + 1
    corner = np.array([min(x0, x1), min(z0, z1)]) if frame[6] > 0 else np.array([min(x0, x1), max(z0, z1)])
    free = np.stack([rng.uniform(x0 - 0.2 * span, x1 + 0.2 * span, (n_free, per)), rng.uniform(z0 - 0.2 * span, z1 + 0.2 * span, (n_free, per))], -1)
    reach = 1.5 * one
    stack = corner + rng.uniform(-reach, reach, (n_stack, per, 2))  # around texel (0, 0): the first tile's list is long
    xz = np.concatenate([free, stack]).reshape(-1, 2).astype(f32)
    n = len(xz)
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), rng.uniform(0.3, 1.0, (n, 1))], 1).astype(f32)
    indices = np.arange(n, dtype=np.uint32)
    features = np.repeat(np.arange((n_free + n_stack + 2) // 3), 3)[: n_free + n_stack].repeat(per).astype(np.uint32)  # three primitives a feature
    width = {"points": 5.0 * one, "lines": 2.5 * one, "triangles": 0.0}[kind]
    return xz, rgba, indices, features, width


# (canvas rows x cols, DEM, registration): what tests/test_gpu_paint.py runs on the device
CASES = [((1, 1), SQUARE, "area"), ((7, 9), SQUARE, "point"), ((16, 16), ANISO, "area"), ((70, 130), SQUARE, "area"), ((257, 64), ANISO, "flipped"),
         ((70, 130), ANISO, "point")]


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dem,canvas,kind", SCENES, ids=[s[0] for s in SCENES])
def test_texel_centres_are_the_inverse_of_the_drape_registration(harness, name, dem, canvas, kind):
    frame = scene_frame(*dem, canvas, kind)
    got = np.zeros((*canvas, 2), f32)
    harness.paint_centres_run(canvas[0], canvas[1], frame.ctypes.data, got.ctypes.data)
    c, r = np.arange(canvas[1], dtype=f32), np.arange(canvas[0], dtype=f32)
    x = (frame[0] + (((c - frame[5]).astype(f32) / frame[4]).astype(f32) * frame[2]).astype(f32)).astype(f32)
    z = (frame[1] + (((r - frame[7]).astype(f32) / frame[6]).astype(f32) * frame[3]).astype(f32)).astype(f32)
    assert np.array_equal(got[..., 0], np.broadcast_to(x, canvas)) and np.array_equal(got[..., 1], np.broadcast_to(z[:, None], canvas))
    # through drape_coords' arithmetic (float64 here) a centre comes back to its texel index
    tx = (got[..., 0].astype(np.float64) - frame[0]) / frame[2] * frame[4] + frame[5]
    tz = (got[..., 1].astype(np.float64) - frame[1]) / frame[3] * frame[6] + frame[7]
    assert np.abs(tx - c).max() < 1e-3 and np.abs(tz - r[:, None]).max() < 1e-3
    assert harness.paint_ramp_run(frame.ctypes.data) == f32(max(abs(frame[2] / frame[4]), abs(frame[3] / frame[6])))
    assert abs(ref.ramp(frame) - harness.paint_ramp_run(frame.ctypes.data)) < 1e-5


@pytest.mark.parametrize("name,dem,canvas,kind", SCENES, ids=[s[0] for s in SCENES])
def test_triangle_decisions_against_the_reference(harness, name, dem, canvas, kind):
    frame = scene_frame(*dem, canvas, kind)
    centres = np.zeros((*canvas, 2), f32)
    harness.paint_centres_run(canvas[0], canvas[1], frame.ctypes.data, centres.ctypes.data)
    xf, zf = centres[..., 0].astype(np.float64), centres[..., 1].astype(np.float64)
    rng = np.random.default_rng(41)
    tested = banded = wrong = covered = 0
    for _ in range(200):
        v = rng.uniform(-170.0, 170.0, (3, 2)).astype(f32)
        rec = records(v, np.array([1, 1, 1, 1], f32), [0, 1, 2], TRIANGLES)[0]
        cov, _ = host_cov(harness, canvas, frame, rec, TRIANGLES, 0.0)
        # the reference at the f32 centres the body uses (the centres' own rounding is test 1's business)
        inside, _, _, dist = ref.triangle(v, xf, zf)
        clear = dist > ref.TRIANGLE_BAND
        tested += clear.size
        banded += int((~clear).sum())
        wrong += int(((cov > 0) != inside)[clear].sum())
        covered += int(inside.sum())
    print(f"{name}: {tested} texel tests, {banded} inside the {ref.TRIANGLE_BAND} m band, {wrong} wrong decisions outside it, {covered} covered")
    assert covered > 0.05 * tested, "the triangles lie on the canvas"
    assert wrong == 0
    assert banded <= ref.TRIANGLE_BAND_MAX_FRACTION * tested


@pytest.mark.parametrize("name,dem,canvas,kind", SCENES, ids=[s[0] for s in SCENES])
def test_stroke_coverage_against_the_reference(harness, name, dem, canvas, kind):
    frame = scene_frame(*dem, canvas, kind)
    centres = np.zeros((*canvas, 2), f32)
    harness.paint_centres_run(canvas[0], canvas[1], frame.ctypes.data, centres.ctypes.data)
    x, z = centres[..., 0].astype(np.float64), centres[..., 1].astype(np.float64)
    one = float(harness.paint_ramp_run(frame.ctypes.data))
    rng = np.random.default_rng(42)
    worst = worst_t = 0.0
    partial = 0
    for i in range(120):
        a, b = rng.uniform(-170.0, 170.0, (2, 2)).astype(f32)
        if i % 6 == 0:
            b = a  # a disc
        hw = f32(rng.uniform(0.0, 25.0)) if i % 5 else f32(0.0)
        rec = records(np.stack([a, b]), np.array([1, 1, 1, 1], f32), [0, 1], LINES)[0]
        cov, par = host_cov(harness, canvas, frame, rec, LINES, hw)
        want, t, _ = ref.segment(a, b, np.float64(hw), one, x, z)
        worst = max(worst, float(np.abs(cov - want).max()))
        on = want > 0
        partial += int(((want > 0) & (want < 1)).sum())
        if on.any():
            worst_t = max(worst_t, float(np.abs(par[..., 0] - t)[on].max()))
        assert cov.min() >= 0.0 and cov.max() <= 1.0
    print(f"{name}: max |cov - cov64| = {worst:.3e}, max |t - t64| where covered = {worst_t:.3e}, {partial} partially covered texels")
    assert partial > 1000
    assert worst <= ref.COVERAGE_TOL
    assert worst_t <= ref.COVERAGE_TOL


@pytest.mark.parametrize("name,dem,canvas,kind", SCENES, ids=[s[0] for s in SCENES])
@pytest.mark.parametrize("prim", ["points", "lines", "triangles"])
def test_blended_values_against_the_reference(harness, name, dem, canvas, kind, prim):
    frame = scene_frame(*dem, canvas, kind)
    xz, rgba, idx, feat, width = case_content(prim, canvas, frame, 7)
    texels = random_canvas(canvas, 3)
    recs = records(xz, rgba, idx, KINDS[prim], feat)
    hw = float(f32(width) * f32(0.5))
    got, vals = host_paint(harness, texels, frame, recs, KINDS[prim], hw, 0.7, values=True)
    # the reference at the centres the body uses, from the values the texels hold
    centres = np.zeros((*canvas, 2), f32)
    harness.paint_centres_run(canvas[0], canvas[1], frame.ctypes.data, centres.ctypes.data)
    exact_frame = frame.astype(np.float64)
    want = ref.paint(unpack(texels), exact_frame, xz, rgba, idx, KINDS[prim], hw, f32(0.7), feat)
    diff = np.abs(vals - want)
    if prim == "triangles":  # a texel in the band of an edge may be decided the other way: left out, and few
        dist = np.full(canvas, np.inf)
        for tri in np.asarray(idx).reshape(-1, 3):
            dist = np.minimum(dist, ref.triangle(xz[tri], centres[..., 0].astype(np.float64), centres[..., 1].astype(np.float64))[3])
        clear = dist > ref.TRIANGLE_BAND
        assert (~clear).sum() <= ref.TRIANGLE_BAND_MAX_FRACTION * clear.size
        diff = diff[clear]
    changed = int((got != texels).sum())
    print(f"{name} {prim}: max |blend - blend64| = {diff.max():.3e}; {changed} of {texels.size} texels changed")
    assert changed > min(texels.size // 4, 50)
    assert diff.max() <= ref.BLEND_TOL
    assert np.array_equal(got, contract_pack(vals)), "the stored texel is the packed value"


# ---- 2. what vector data needs ---------------------------------------------------------------------------------------------------------
def mesh(frame, canvas, snapped, seed=5, n=9):
    """An n x n-vertex triangulated grid over the middle of the canvas, interior vertices jittered (or snapped to texel centres):
    128 triangles for n = 9."""
    rng = np.random.default_rng(seed)
    cols = np.linspace(0.15 * canvas[1], 0.85 * canvas[1], n)
    rows = np.linspace(0.15 * canvas[0], 0.85 * canvas[0], n)
    gc, gr = np.meshgrid(cols, rows)
    inner = np.zeros((n, n), bool)
    inner[1:-1, 1:-1] = True
    gc = gc + inner * rng.uniform(-0.3, 0.3, (n, n)) * (cols[1] - cols[0])
    gr = gr + inner * rng.uniform(-0.3, 0.3, (n, n)) * (rows[1] - rows[0])
    if snapped:
        gc, gr = np.rint(gc), np.rint(gr)
    ox, oz, sx, sz, kx, bx, kz, bz = (np.float64(v) for v in frame)
    if snapped:  # exactly the f32 centres
        vx = (frame[0] + (((gc.astype(f32) - frame[5]).astype(f32) / frame[4]).astype(f32) * frame[2]).astype(f32)).astype(f32)
        vz = (frame[1] + (((gr.astype(f32) - frame[7]).astype(f32) / frame[6]).astype(f32) * frame[3]).astype(f32)).astype(f32)
    else:
        vx, vz = (ox + (gc - bx) / kx * sx).astype(f32), (oz + (gr - bz) / kz * sz).astype(f32)
    xz = np.stack([vx.ravel(), vz.ravel()], 1)
    tri = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            tri += ([a, b, d, a, d, c] if (i + j) % 2 else [a, b, c, b, d, c])  # both diagonals, both windings below
    tri = np.array(tri, np.uint32).reshape(-1, 3)
    tri[::3] = tri[::3, ::-1]  # every third triangle wound the other way
    lo_c, hi_c, lo_r, hi_r = cols[0] + 1.5, cols[-1] - 1.5, rows[0] + 1.5, rows[-1] - 1.5
    c, r = np.meshgrid(np.arange(canvas[1]), np.arange(canvas[0]))
    interior = (c > lo_c) & (c < hi_c) & (r > lo_r) & (r < hi_r)
    outside = (c < cols[0] - 1.5) | (c > cols[-1] + 1.5) | (r < rows[0] - 1.5) | (r > rows[-1] + 1.5)
    return xz, tri.ravel(), interior, outside


@pytest.mark.parametrize("name,dem,canvas,kind", SCENES, ids=[s[0] for s in SCENES])
@pytest.mark.parametrize("snapped", [False, True], ids=["jittered", "snapped"])
def test_a_triangle_mesh_is_watertight(harness, name, dem, canvas, kind, snapped):
    frame = scene_frame(*dem, canvas, kind)
    xz, idx, interior, outside = mesh(frame, canvas, snapped)
    assert len(idx) // 3 == 128 and interior.sum() > 0.3 * interior.size
    base = np.array([0.25, 0.5, 0.75], f32)
    colour = np.array([1.0, 0.5, 0.0, 1.0], f32)
    texels = contract_pack(np.broadcast_to(base, (*canvas, 3)).copy())
    # a feature per triangle: ids are read at first vertices, so the vertices are duplicated per triangle
    tri = idx.reshape(-1, 3)
    xz_t, idx_t = xz[tri].reshape(-1, 2), np.arange(tri.size, dtype=np.uint32)
    feat_t = np.repeat(np.arange(len(tri), dtype=np.uint32), 3)
    recs = records(xz_t, colour, idx_t, TRIANGLES, feat_t)
    assert len(set(recs["feature"])) == 128
    for tiled in (0, 1):
        got = host_paint(harness, texels, frame, recs, TRIANGLES, 0.0, 0.5, tiled=tiled)
        once = contract_pack((base + f32(0.5) * (colour[:3] - base)).reshape(1, 1, 3))[0, 0]
        assert (got[interior] == once).all(), f"{int((got[interior] != once).sum())} interior texels are not blended exactly once"
        assert (got[outside] == texels[outside]).all()
        assert set(np.unique(got)) <= {once, texels[0, 0]}, "every texel is blended once or not at all"


def zigzag(frame, canvas, n=12):
    x0, x1, z0, z1 = extent(frame, canvas)
    xs = np.linspace(x0 + 0.1 * (x1 - x0), x1 - 0.1 * (x1 - x0), n)
    zs = np.where(np.arange(n) % 2 == 0, z0 + 0.3 * (z1 - z0), z0 + 0.7 * (z1 - z0))
    return np.stack([xs, zs], 1).astype(f32)


@pytest.mark.parametrize("name,dem,canvas,kind", SCENES, ids=[s[0] for s in SCENES])
def test_one_feature_blends_once(harness, name, dem, canvas, kind):
    frame = scene_frame(*dem, canvas, kind)
    xz = zigzag(frame, canvas)
    strip = np.stack([np.arange(len(xz) - 1), np.arange(1, len(xz))], 1).ravel()
    base, colour = np.array([0.75, 0.75, 0.75], f32), np.array([0.0, 0.0, 0.0, 1.0], f32)
    texels = contract_pack(np.broadcast_to(base, (*canvas, 3)).copy())
    one = ref.ramp(frame)
    hw = float(f32(3.0 * one))
    got = host_paint(harness, texels, frame, records(xz, colour, strip, LINES), LINES, hw, 0.5)
    once = contract_pack((base + f32(0.5) * (colour[:3] - base)).reshape(1, 1, 3))[0, 0]
    values = unpack(got)[..., 0]
    assert (got == once).sum() > 200 and values.min() == unpack(np.array([[once]]))[0, 0, 0], "no texel is darker than once blended"
    # the joints are where it would show: around every inner vertex the full-coverage texels hold the once-blended value
    x, z = ref.centres(canvas[0], canvas[1], frame)
    for v in xz[1:-1]:
        near = np.hypot(x - v[0], z - v[1]) < hw - one
        assert near.any() and (got[near] == once).all()
    # the same strip as a feature per segment does blend twice at the joints: the test can tell
    per_segment = np.repeat(np.arange(len(xz)), 1).astype(np.uint32)
    twice = host_paint(harness, texels, frame, records(xz, colour, strip, LINES, per_segment), LINES, hw, 0.5)
    assert unpack(twice)[..., 0].min() < values.min()


def test_the_later_feature_wins_and_one_call_equals_two(harness):
    _, dem, canvas, kind = SCENES[0]
    frame = scene_frame(*dem, canvas, kind)
    one = ref.ramp(frame)
    xz = np.array([[-20.0, 0.0], [20.0, 0.0]], f32)
    rgba = np.array([[1, 0, 0, 1], [0, 0, 1, 1]], f32)
    texels = random_canvas(canvas, 9)
    hw = float(f32(40.0))
    both = host_paint(harness, texels, frame, records(xz, rgba, [0, 1], POINTS, np.array([0, 1])), POINTS, hw, 1.0)
    x, z = ref.centres(canvas[0], canvas[1], frame)
    overlap = (np.hypot(x + 20, z) < hw - one) & (np.hypot(x - 20, z) < hw - one)
    only_first = (np.hypot(x + 20, z) < hw - one) & (np.hypot(x - 20, z) > hw + one)
    assert overlap.sum() > 50 and only_first.sum() > 50
    assert (unpack(both)[overlap] == np.array([0, 0, 1], f32)).all() and (unpack(both)[only_first] == np.array([1, 0, 0], f32)).all()
    swapped = host_paint(harness, texels, frame, records(xz[::-1], rgba[::-1], [0, 1], POINTS, np.array([0, 1])), POINTS, hw, 1.0)
    assert (unpack(swapped)[overlap] == np.array([1, 0, 0], f32)).all()
    # as ONE feature the nearer disc's colour counts (highest coverage, ties to the lowest index), blended once
    single = host_paint(harness, texels, frame, records(xz, rgba, [0, 1], POINTS), POINTS, hw, 1.0)
    assert (unpack(single)[overlap] == np.array([1, 0, 0], f32)).all()
    # two calls, one feature each, are the one call with two features: texels are binary16 between calls, and these values are exact
    first = host_paint(harness, texels, frame, records(xz[:1], rgba[:1], [0], POINTS), POINTS, hw, 1.0)
    second = host_paint(harness, first, frame, records(xz[1:], rgba[1:], [0], POINTS), POINTS, hw, 1.0)
    full = (np.hypot(x + 20, z) < hw - one) | (np.hypot(x - 20, z) < hw - one)
    assert np.array_equal(second[full], both[full])


def test_degenerate_primitives_and_untouched_texels(harness):
    _, dem, canvas, kind = SCENES[0]
    frame = scene_frame(*dem, canvas, kind)
    texels = random_canvas(canvas, 10)
    red = np.array([1, 0, 0, 1], f32)
    # zero area: three points on a line, two equal vertices, three equal vertices
    for tri in ([[0, 0], [10, 10], [20, 20]], [[0, 0], [0, 0], [30, 5]], [[5, 5], [5, 5], [5, 5]], [[-40, 0], [40, 0], [0, 0]]):
        got = host_paint(harness, texels, frame, records(np.array(tri, f32), red, [0, 1, 2], TRIANGLES), TRIANGLES, 0.0, 1.0)
        assert np.array_equal(got, texels), tri
    # a == b is the disc a point paints
    p = np.array([[12.5, -30.0]], f32)
    disc = host_paint(harness, texels, frame, records(p, red, [0], POINTS), POINTS, 17.0, 0.8)
    same = host_paint(harness, texels, frame, records(np.repeat(p, 2, 0), red, [0, 1], LINES), LINES, 17.0, 0.8)
    assert np.array_equal(disc, same) and (disc != texels).sum() > 100
    x, z = ref.centres(canvas[0], canvas[1], frame)
    d = np.hypot(x - 12.5, z + 30.0)
    one = ref.ramp(frame)
    assert (disc != texels)[d < 17.0 - one].all() and np.array_equal(disc[d > 17.0 + one], texels[d > 17.0 + one]), "untouched texels keep their bits"
    # off the canvas, on every side and far away: nothing changes, whatever the kind
    for off in ([-900.0, 0.0], [900.0, 0.0], [0.0, -900.0], [0.0, 900.0], [3e30, -3e30], [1e38, 1e38]):
        v = (np.array([[0, 0], [15, 3], [4, 12]], f32) + np.array(off, f32)).astype(f32)
        for k, idx in ((POINTS, [0, 1, 2]), (LINES, [0, 1, 1, 2]), (TRIANGLES, [0, 1, 2])):
            for tiled in (0, 1):
                got = host_paint(harness, texels, frame, records(v, red, idx, k), k, 20.0, 1.0, tiled=tiled)
                assert np.array_equal(got, texels), (off, k, tiled)
    # zero opacity, zero alpha: every bit stays
    v = np.array([[-100, -100], [100, 90], [-80, 100]], f32)
    assert np.array_equal(host_paint(harness, texels, frame, records(v, red, [0, 1, 2], TRIANGLES), TRIANGLES, 0.0, 0.0), texels)
    clear = np.array([1, 0, 0, 0], f32)
    assert np.array_equal(host_paint(harness, texels, frame, records(v, clear, [0, 1, 1, 2], LINES), LINES, 9.0, 1.0), texels)


# ---- 3. binning -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas,dem,kind", CASES, ids=lambda v: v if isinstance(v, str) else None)
@pytest.mark.parametrize("prim", ["points", "lines", "triangles"])
def test_binning_is_conservative_and_the_tiled_walk_returns_the_same_bits(harness, canvas, dem, kind, prim):
    frame = scene_frame(*dem, canvas, kind)
    xz, rgba, idx, feat, width = case_content(prim, canvas, frame, 11)
    k = KINDS[prim]
    hw = float(f32(width) * f32(0.5))
    recs = records(xz, rgba, idx, k, feat)
    bins = host_bins(harness, canvas, frame, recs, k, hw)
    tiles_x = (canvas[1] + 15) // 16
    r, c = np.meshgrid(np.arange(canvas[0]), np.arange(canvas[1]), indexing="ij")
    tile_of = (r // 16) * tiles_x + c // 16
    listed = 0
    for rec, tiles in zip(recs, bins):
        assert (np.diff(tiles.astype(np.int64)) > 0).all(), "rising order, every tile once"
        cov, _ = host_cov(harness, canvas, frame, rec, k, hw)
        need = set(np.unique(tile_of[cov > 0]).tolist())
        assert need <= set(tiles.tolist()), f"tiles {sorted(need - set(tiles.tolist()))} hold covered texels and are not listed"
        listed += len(tiles)
    assert max(len(t) for t in bins) >= 1
    texels = random_canvas(canvas, 12)
    whole = host_paint(harness, texels, frame, recs, k, hw, 0.6)
    assert np.array_equal(host_paint(harness, texels, frame, recs, k, hw, 0.6, tiled=1), whole)
    assert (whole != texels).any()
    first = sum(1 for t in bins if 0 in t.tolist())
    assert first > 128, f"{first} primitives over the first tile: more than two LDS chunks"


def far_content(kind, shape, frame, seed):
    """Primitives whose vertices lie up to the contract's reach (2^16 texels from the terrain's centre) away and which cross the
    canvas: where the f32 distance is coarsest.  (xz, rgba, indices, features, width)."""
    rng = np.random.default_rng(seed)
    one = ref.ramp(frame)
    reach = 65536.0 * one
    x0, x1, z0, z1 = extent(frame, shape)
    n = 24
    inside = np.stack([rng.uniform(min(x0, x1), max(x0, x1), n), rng.uniform(min(z0, z1), max(z0, z1), n)], 1)
    angle = rng.uniform(0.0, 2.0 * np.pi, n)
    far = np.clip(inside + (rng.uniform(0.3, 0.99, n) * reach)[:, None] * np.stack([np.cos(angle), np.sin(angle)], 1), -0.99 * reach, 0.99 * reach)
    if kind == "lines":  # from far away through a point of the canvas and on to the other side
        xz = np.stack([far, inside + 0.5 * (inside - far)], 1).reshape(-1, 2)
    else:  # slivers and wedges with one far vertex
        third = inside + rng.uniform(-40.0, 40.0, (n, 2)) * one
        xz = np.stack([inside, far, third], 1).reshape(-1, 2)
    xz = np.clip(xz, -0.99 * reach, 0.99 * reach).astype(f32)
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (len(xz), 3)), rng.uniform(0.4, 1.0, (len(xz), 1))], 1).astype(f32)
    per = KINDS[kind] + 1
    return xz, rgba, np.arange(len(xz), dtype=np.uint32), np.repeat(np.arange(n), per).astype(np.uint32), (3.0 * one if kind == "lines" else 0.0)


@pytest.mark.parametrize("canvas,dem,kind", [CASES[3], CASES[4]], ids=["square-70x130", "aniso-257x64-flipped"])
@pytest.mark.parametrize("prim", ["lines", "triangles"])
def test_vertices_out_to_the_reach_are_binned_conservatively(harness, canvas, dem, kind, prim):
    frame = scene_frame(*dem, canvas, kind)
    k = KINDS[prim]
    r, c = np.meshgrid(np.arange(canvas[0]), np.arange(canvas[1]), indexing="ij")
    tile_of = (r // 16) * ((canvas[1] + 15) // 16) + c // 16
    texels = random_canvas(canvas, 14)
    for seed in range(6):
        xz, rgba, idx, feat, width = far_content(prim, canvas, frame, 50 + seed)
        assert np.abs(xz).max() > 20000.0 * ref.ramp(frame)
        hw = float(f32(width) * f32(0.5))
        recs = records(xz, rgba, idx, k, feat)
        covered = 0
        for rec, tiles in zip(recs, host_bins(harness, canvas, frame, recs, k, hw)):
            cov, _ = host_cov(harness, canvas, frame, rec, k, hw)
            covered += int((cov > 0).sum())
            assert set(np.unique(tile_of[cov > 0]).tolist()) <= set(tiles.tolist())
        assert covered > 200, "the far primitives do cross the canvas"
        whole = host_paint(harness, texels, frame, recs, k, hw, 0.8)
        assert np.array_equal(host_paint(harness, texels, frame, recs, k, hw, 0.8, tiled=1), whole)


def test_a_long_diagonal_lists_the_tiles_along_it_not_its_box(harness):
    dem, canvas = SQUARE, (512, 512)
    frame = scene_frame(*dem, canvas, "area")
    x0, x1, z0, z1 = extent(frame, canvas)
    xz = np.array([[x0, z0], [x1, z1]], f32)
    recs = records(xz, np.array([1, 1, 1, 1], f32), [0, 1], LINES)
    one = ref.ramp(frame)
    (tiles,) = host_bins(harness, canvas, frame, recs, LINES, float(f32(one)))
    assert 32 <= len(tiles) <= 4 * 32, f"{len(tiles)} of {32 * 32} tiles listed for the diagonal of a 32 x 32-tile canvas"
    cov, _ = host_cov(harness, canvas, frame, recs[0], LINES, float(f32(one)))
    r, c = np.nonzero(cov > 0)
    assert set(((r // 16) * 32 + c // 16).tolist()) <= set(tiles.tolist())


# ---- 4. the C ABI, the wrapper, the facade ---------------------------------------------------------------------------------------------
FIELDS = ("flags", "primitive", "vertex_count", "xz", "rgba", "feature", "indices", "index_count", "half_width", "opacity", "aim")


def test_header_ctypes_table_and_descriptor_layout_agree(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert re.search(r"\bf3d_session_paint\s*\(", header) and re.search(r"\bf3d_session_drape_read\s*\(", header)
    names = {n for n, _, _ in _native.ABI}
    assert "f3d_session_paint" in names and "f3d_session_drape_read" in names
    assert "#define F3D_ABI_VERSION 6u" in header and _native.ABI_VERSION == 6  # additive: detected by the symbol
    for name, value in (("POINTS", 0), ("LINES", 1), ("TRIANGLES", 2), ("MAX_PRIMITIVES", 1 << 24)):
        assert re.search(rf"#define F3D_PAINT_{name} {value}u\b", header), name
        assert getattr(_native, f"PAINT_{name}") == value
    D = _native.PaintDesc
    assert [n for n, _ in D._fields_] == ["struct_size", *FIELDS]
    out = (C.c_uint32 * 32)()
    n = harness.paint_desc_layout(out, 32)
    assert n == 2 + len(FIELDS) + 3
    assert list(out[:n - 3]) == [C.sizeof(D), D.struct_size.offset, *(getattr(D, f).offset for f in FIELDS)]
    assert list(out[n - 3:n]) == [PRIM.itemsize, 16, 64] and PRIM.itemsize == 80
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f3d_terrain_pt.h"\nint main(void) { printf("%zu ' + " ".join(["%zu"] * len(FIELDS)) + \
          '\\n", sizeof(f3d_session_paint_desc), ' + ", ".join(f"offsetof(f3d_session_paint_desc, {f})" for f in FIELDS) + "); return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:  # (the header as a C compiler reads it)
        c = Path(tmp) / "layout.c"
        c.write_text(src)
        exe = Path(tmp) / "layout"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(D), *(getattr(D, f).offset for f in FIELDS)]
    listing = subprocess.run(["nm", "-D", "--defined-only", str(_native.library_path())], capture_output=True, text=True, check=True)
    for symbol in ("f3d_session_paint", "f3d_session_drape_read"):
        assert any(line.split()[-1] == symbol and " T " in line for line in listing.stdout.splitlines()), symbol
    assert "f3d_paint.hip" in _native.HIP_SOURCES


def test_the_wrapper_checks_its_arguments_before_the_native_call():
    s = _bare_session((33, 33))
    xz = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], f32)
    red = (1.0, 0.0, 0.0, 1.0)
    try:
        with pytest.raises(ValueError, match="primitive must be 'points', 'lines' or 'triangles', got 'quads'"):
            s.paint(xz, red, primitive="quads")
        with pytest.raises(ValueError, match=re.escape("xz must have shape (N, 2) with N >= 1, got (4, 3)")):
            s.paint(np.zeros((4, 3), f32), red)
        with pytest.raises(ValueError, match=re.escape("xz must have shape (N, 2) with N >= 1, got (0, 2)")):
            s.paint(np.zeros((0, 2), f32), red)
        with pytest.raises(ValueError, match="rgba must be one colour of 3 or 4 numbers or have shape"):
            s.paint(xz, np.zeros((3, 4), f32))
        with pytest.raises(ValueError, match="rgba must be one colour of 3 or 4 numbers or have shape"):
            s.paint(xz, (1.0, 0.0))
        with pytest.raises(ValueError, match="indices must be integers"):
            s.paint(xz, red, [0.0, 1.0])
        with pytest.raises(ValueError, match="indices must not be negative"):
            s.paint(xz, red, [0, -1])
        with pytest.raises(ValueError, match="3 indices do not make lines"):
            s.paint(xz, red, [0, 1, 2])
        with pytest.raises(ValueError, match="4 indices do not make triangles"):
            s.paint(xz, red, [0, 1, 2, 3], primitive="triangles")
        with pytest.raises(ValueError, match="0 indices do not make lines"):
            s.paint(xz[:1], red)
        with pytest.raises(ValueError, match="index 4 is out of range: the call has 4 vertices"):
            s.paint(xz, red, [0, 4])
        for width in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="width must be finite and >= 0 metres"):
                s.paint(xz, red, width=width)
        for opacity in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match=re.escape("opacity must lie in [0, 1]")):
                s.paint(xz, red, opacity=opacity)
        with pytest.raises(ValueError, match="features must be"):
            s.paint(xz, red, features=[0, 0, 1])
        with pytest.raises(ValueError, match="features must be"):
            s.paint(xz, red, features=[0.5, 0, 1, 1])
        with pytest.raises(TypeError, match="paint\\(\\) got an unexpected keyword argument 'spp'"):
            s.paint(xz, red, spp=4)
        with pytest.raises(OverflowError):
            s.paint(xz, red, seed=-1)
        # what the wrapper accepts gets as far as the native layer
        for args, kw in (((xz, red), {}), ((xz, (0.2, 0.3, 0.4)), dict(primitive="points", width=0.0)), ((xz, np.full((4, 3), 0.5, f32), [0, 1, 2, 0, 2, 3]),
                         dict(primitive="triangles", opacity=0.5, features=[1, 1, 2, 2])), ((xz, red, [[0, 1], [2, 3]]), dict(seed=3))):
            with pytest.raises(AssertionError, match="the device was touched"):
                s.paint(*args, **kw)
        assert s.paint_indices(4, "lines").tolist() == [0, 1, 1, 2, 2, 3] and s.paint_indices(4, "points").tolist() == [0, 1, 2, 3]
        assert s.paint_indices(7, "triangles").tolist() == [0, 1, 2, 3, 4, 5] and s.paint_indices(1, "lines").tolist() == []
    finally:
        s._handle = None


def _decode(rows):
    return [[float(v) if isinstance(v, str) and i < 7 else (float(v) if v == "nan" else v) for i, v in enumerate(r)] for r in rows]


def test_the_facade_validates_vertices_with_the_reference_messages():
    from forge3d_amd.viewer import ViewerHandle

    fixture = json.loads((ROOT / "tests" / "golden" / "vector_overlay_messages.json").read_text())
    assert len(fixture["cases"]) >= 15 and sum("message" in c for c in fixture["cases"]) >= 10
    for case in fixture["cases"]:
        rows = _decode(case["vertices"])
        if "message" in case:
            with pytest.raises(ValueError) as err:
                ViewerHandle.vector_overlay_vertices(rows)
            assert str(err.value) == case["message"], case["name"]
        else:
            got = ViewerHandle.vector_overlay_vertices(rows)
            assert got.shape == (len(rows), 8) and got.tolist() == [[float(v) for v in r] for r in case["returns"]], case["name"]


def test_the_facade_expands_strips_orders_layers_and_refuses_what_has_no_offline_form():
    from forge3d_amd.viewer import ViewerError, ViewerHandle

    v = ViewerHandle(96, 64)
    rows = [[float(i), 99.0, float(-i), 0.1, 0.2, 0.3, 1.0, i // 2] for i in range(6)]
    assert ViewerHandle.expand_strip([0, 1, 2, 3], "line_strip")[0] == "lines"
    assert ViewerHandle.expand_strip([0, 1, 2, 3], "line_strip")[1].tolist() == [0, 1, 1, 2, 2, 3]
    kind, tri = ViewerHandle.expand_strip([0, 1, 2, 3, 4], "triangle_strip")
    assert kind == "triangles" and tri.tolist() == [0, 1, 2, 2, 1, 3, 2, 3, 4]
    assert ViewerHandle.expand_strip([3, 1, 2], "triangles")[1].tolist() == [3, 1, 2]
    with pytest.raises(ViewerError, match="drape=False"):
        v.add_vector_overlay("roads", rows, [0, 1], "lines", drape=False)
    with pytest.raises(ViewerError, match="primitive must be one of"):
        v.add_vector_overlay("roads", rows, [0, 1], "quads")
    with pytest.raises(ViewerError, match=re.escape("indices must lie in [0, 6)")):
        v.add_vector_overlay("roads", rows, [0, 6], "lines")
    with pytest.raises(ViewerError, match="2 indices do not make triangles"):
        v.add_vector_overlay("roads", rows, [0, 1], "triangles")
    with pytest.raises(ViewerError, match=re.escape("opacity must lie in [0, 1]")):
        v.add_vector_overlay("roads", rows, [0, 1], "lines", opacity=2.0)
    with pytest.raises(ValueError, match="vector vertex 0 must contain exactly 8 lanes"):
        v.add_vector_overlay("roads", [[0.0] * 7], [0], "points")
    assert v.vector_layers() == []
    a = v.add_vector_overlay("parcels", rows, [0, 1, 2, 3], "triangle_strip", opacity=0.5, z_order=5)
    b = v.add_vector_overlay("roads", rows, [0, 1, 2], "line_strip", line_width=3.0, z_order=-1)
    c = v.add_vector_overlay("peaks", rows, [4, 5], "points", point_size=7.0, z_order=5)
    assert (a, b, c) == (1, 2, 3)
    assert [layer["name"] for layer in v.vector_layers()] == ["roads", "parcels", "peaks"], "(z_order, id)"
    roads, parcels, peaks = v.vector_layers()
    assert roads["primitive"] == "lines" and roads["indices"].tolist() == [0, 1, 1, 2] and roads["texels"] == 3.0
    assert parcels["primitive"] == "triangles" and parcels["indices"].tolist() == [0, 1, 2, 2, 1, 3] and parcels["opacity"] == 0.5
    assert peaks["primitive"] == "points" and peaks["texels"] == 7.0
    assert roads["xz"].tolist() == [[float(i), float(-i)] for i in range(6)], "Y is ignored: X, Z are world x, z"
    assert roads["features"].tolist() == [0, 0, 1, 1, 2, 2] and roads["rgba"].dtype == np.float32
    v.remove_vector_overlay(a)
    assert [layer["name"] for layer in v.vector_layers()] == ["roads", "peaks"]
    with pytest.raises(ViewerError, match="no vector overlay with id 1"):
        v.remove_vector_overlay(a)
    assert v.add_vector_overlay("more", rows, [0], "points") == 4, "ids are not reused"
    assert v.vector_canvas_shape((33, 17)) == (128, 64) and v.vector_canvas_shape((4097, 4097)) == (8192, 8192)
    v.set_vector_canvas(300, 200)
    assert v.vector_canvas_shape((33, 17)) == (300, 200)
    v.set_vector_canvas(None)
    assert v.vector_canvas_shape((33, 17)) == (128, 64)
    with pytest.raises(ViewerError, match="1..16384 texels a side"):
        v.set_vector_canvas(0, 5)
    with pytest.raises(ViewerError, match="belongs to the interactive raster viewer"):
        v.add_label("x", (0, 0, 0))


def test_the_stroke_of_paint_is_refused_in_the_words_the_derived_paints_share():
    from test_session_contour_host import refused

    s = _bare_session((33, 33))
    xz, red = np.array([[0, 0], [10, 0]], f32), (1.0, 0.0, 0.0, 1.0)
    refused("width must be finite and >= 0 metres, got -1.0", s.paint, xz, red, width=-1.0)
    refused("width must be finite and >= 0 metres, got nan", s.paint, xz, red, width=float("nan"))
    refused("width must be finite and >= 0 metres, got -1.0", s.paint, xz, red, width=-1.0, opacity=1.5)  # (the width's fault wins)
    refused("opacity must lie in [0, 1], got 1.5", s.paint, xz, red, opacity=1.5)
    refused("rgba must be one colour of 3 or 4 numbers or have shape (2, 3|4), got (2,)", s.paint, xz, (1.0, 0.0))  # (its colours stay its own)
    refused("rgba must be one colour of 3 or 4 numbers or have shape (2, 3|4), got (5,)", s.paint, xz, (1.0, 0.0, 0.0, 1.0, 0.5), width=-1.0)
