"""Irradiation rasters on a live terrain session (f3d_session_irradiation), the parts that need no GPU.

The lane body of the irradiation kernel (csrc/f3d_irradiation.h, what k_irradiation runs per lane) compiled for the host
(tests/irradiation_host) and run over whole 64-lane waves of the emulator's fibers, against the contract restated here in
NumPy -- gradient, cosine and the sequential f32 sum, one rounding per operation, plane_at's single rounding through f64 --
with the lit bits taken from ``contract_bits`` (tests/test_session_raster_host.py: the oracle's terrain trace).

* energy, count and normals equal bit for bit, nothing left out: DEMs 5x3, 33x33, 64x64, 65x63, curved on and off, HORIZONTAL
  on and off, regions with nonzero row0 / col0, a 1x1 region, K = 1, 3, 8; every shape holds self-shadowed, blocked and lit
  terms, so nothing passes by marching nothing;
* no march for a facet turned away, a weight that is not positive, a NaN component (the device form's path), a zero direction;
* the planar incline against the analytic normal in f64 (a counted bound);
* the header, the ctypes table and the descriptor's layout; the wrapper's argument checks; sun_track and clear_sky;
* a stand-alone driver (its own main) of the same lane body built with -fsanitize=address,undefined and run once.
"""
from __future__ import annotations

import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from emul import emul
from forge3d_amd import geo, insolation
from test_session_raster_host import ALONG, SHAPES, HostScene, _kw, _planar, contract_bits, contract_origins, plane_at, shaped_dem, sun_direction

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "irradiation_host" / "irradiation_harness.cpp"
TERRAIN_ONLY, CURVED, HORIZONTAL = 1, 2, 16
f32 = np.float32

# the issue's eight sun positions (azimuth, elevation), with unequal weights
SUNS = [(90, 4), (110, 15), (135, 30), (180, 50), (225, 30), (250, 15), (270, 4), (0, 20)]
WEIGHTS = [120.0, 310.5, 640.25, 905.0, 633.0, 298.75, 111.5, 57.0]


def directions(k=8):
    d = np.stack([sun_direction(az, el) for az, el in SUNS]).astype(f32)
    d[:, 3] = f32(WEIGHTS)
    return d[:k].copy()


class _AsRaster:
    """HostScene (tests/test_session_raster_host.py) asks its library for raster_scene_create / raster_scene_destroy."""

    def __init__(self, lib):
        self.raster_scene_create, self.raster_scene_destroy = lib.irradiation_scene_create, lib.irradiation_scene_destroy


class Scene(HostScene):
    """A scene as the emulator sets it up, and irradiation rasters over it as f3d_session_irradiation's device form answers."""

    def __init__(self, lib, dem, kw, **more):
        super().__init__(_AsRaster(lib), dem, kw, **more)
        self.irr = lib

    def irradiation(self, terms, flags=0, region=None, lift=1e-3):
        row0, col0, rows, cols = self.region(region)
        n = rows * cols
        terms = np.ascontiguousarray(terms, f32).reshape(-1, 4)
        k = len(terms)
        energy, count = np.full(n, 77, f32), np.full(n, 77, np.uint32)
        normal, marches, origins = np.full((n, 3), 77, f32), np.full((max(k, 1), n), 77, np.uint32), np.full((n, 3), 77, f32)
        assert self.irr.irradiation_run(self.handle, flags, row0, col0, rows, cols, float(lift), k, terms.ctypes.data if k else None,
                                        energy.ctypes.data, count.ctypes.data, normal.ctypes.data, marches.ctypes.data, origins.ctypes.data) == 0
        return {"energy": energy.reshape(rows, cols), "count": count.reshape(rows, cols), "normal": normal.reshape(rows, cols, 3),
                "marches": marches[:k].reshape(k, rows, cols), "origins": origins.reshape(rows, cols, 3)}


def load_harness():
    lib = emul.build_harness(HARNESS, "irradiation_host")
    lib.irradiation_scene_create.restype = C.c_void_p
    lib.irradiation_scene_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.irradiation_scene_destroy.argtypes = [C.c_void_p]
    lib.irradiation_run.restype = C.c_int
    lib.irradiation_run.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_float, C.c_uint32] + [C.c_void_p] * 6
    lib.irradiation_desc_size.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def irradiation_harness():
    return load_harness()


def shaped_kw(dem):
    """The golden scene's own sample spacing (its 64 samples across the span) under every crop of its relief: the slopes, and
    with them the self-shadowed and the blocked terms, are the golden DEM's on the 5x3 crop too."""
    import scenes

    kw = _kw(dem)
    kw["spacing"] = (scenes.SPAN / 63.0, scenes.SPAN / 63.0)
    return kw


@pytest.fixture(scope="module")
def irradiation_scenes(irradiation_harness):
    made = {}
    for shape in SHAPES:
        dem = shaped_dem(shape)
        made[shape] = Scene(irradiation_harness, dem, shaped_kw(dem))
    yield made
    for s in made.values():
        s.close()


# ---- the contract, restated in NumPy -----------------------------------------------------------------------------------------
def contract_slope(scene, region, horizontal):
    """(gx, gz, q), f32 (rows, cols) each, of the region: central differences of the heights the session holds, one-sided on
    the border, over the lattice's own plane positions."""
    row0, col0, rows, cols = region
    if horizontal:
        zero = np.zeros((rows, cols), f32)
        return zero, zero.copy(), np.ones((rows, cols), f32)
    h = np.asarray(scene.dem, f32) * f32(scene.kw["exaggeration"])
    dem_h, dem_w = h.shape
    j, i = np.meshgrid(np.arange(row0, row0 + rows), np.arange(col0, col0 + cols), indexing="ij")
    iW, iE = np.where(i > 0, i - 1, i), np.where(i + 1 < dem_w, i + 1, i)
    jN, jS = np.where(j > 0, j - 1, j), np.where(j + 1 < dem_h, j + 1, j)
    run_x = plane_at(scene.origin[0], iE, scene.spacing[0]) - plane_at(scene.origin[0], iW, scene.spacing[0])
    run_z = plane_at(scene.origin[1], jS, scene.spacing[1]) - plane_at(scene.origin[1], jN, scene.spacing[1])
    gx = (h[j, iE] - h[j, iW]) / run_x
    gz = (h[jS, i] - h[jN, i]) / run_z
    q = (gx * gx + gz * gz) + f32(1.0)
    assert gx.dtype == f32 and gz.dtype == f32 and q.dtype == f32
    return gx, gz, q


def contract_normals(slope):
    gx, gz, q = slope
    length = np.sqrt(q)
    return np.stack([-gx / length, f32(1.0) / length, -gz / length], -1).astype(f32)


def contract_terms(scene, slope, o, terms):
    """Per direction k: the cosine c (K, rows, cols) f32 and `go` -- False: settled without a ray."""
    gx, gz, q = slope
    cs, gos = [], []
    finite_o = np.isfinite(o).all(-1)
    with np.errstate(all="ignore"):
        for x, y, z, wt in np.asarray(terms, f32).reshape(-1, 4):
            l2 = (x * x + y * y) + z * z
            m = (y - gx * x) - gz * z
            c = m / np.sqrt(q * l2)
            good = finite_o & bool(np.isfinite([x, y, z]).all() and l2 > 0 and np.isfinite(l2))
            cs.append(c.astype(f32))
            gos.append(good & bool(wt > 0) & (c > 0))
    assert all(c.dtype == f32 for c in cs)
    return np.stack(cs), np.stack(gos)


def contract_irradiation(scene, terms, curved, horizontal=False, region=None, lift=1e-3, bits=None):
    """What the contract asks for: energy, count, normal, and `go`, `bits` (K, rows, cols).  bits: the oracle's (contract_bits)
    unless handed in."""
    region = scene.region(region)
    terms = np.asarray(terms, f32).reshape(-1, 4)
    slope = contract_slope(scene, region, horizontal)
    o = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, region, lift)
    c, go = contract_terms(scene, slope, o, terms)
    if bits is None:
        bits = contract_bits(scene, ALONG, terms, curved, region, lift)
    energy, count = np.zeros(region[2:], f32), np.zeros(region[2:], np.uint32)
    for k in range(len(terms)):  # the sequential f32 sum: sum = sum + wt * c
        lit = go[k] & bits[k]
        energy = np.where(lit, energy + terms[k, 3] * c[k], energy).astype(f32)
        count = count + lit.astype(np.uint32)
    return {"energy": energy, "count": count, "normal": contract_normals(slope), "go": go, "bits": bits, "c": c}


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(scene, terms, curved, horizontal=False, region=None, lift=1e-3):
    got = scene.irradiation(terms, (CURVED if curved else 0) | (HORIZONTAL if horizontal else 0), region, lift)
    want = contract_irradiation(scene, terms, curved, horizontal, region, lift)
    wrong = int((got["energy"].view(np.uint32) != want["energy"].view(np.uint32)).sum())
    assert wrong == 0, f"{wrong} of {want['energy'].size} energies differ from the contract"
    assert np.array_equal(got["count"], want["count"]), "count"
    assert same_bits(got["normal"], want["normal"]), "normals"
    assert not got["marches"][~want["go"]].any(), "a term settled without a ray has no march"
    assert (got["marches"][want["go"]] >= 1).all(), "a term that goes marches"
    return got, want


# ---- 1. the contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("horizontal", [False, True], ids=["slope", "horizontal"])
@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_energy_count_and_normals_equal_the_contract_bit_for_bit(irradiation_scenes, shape, curved, horizontal):
    scene = irradiation_scenes[shape]
    assert scene.kw["exaggeration"] == 20.0 and scene.curvature_enabled
    terms = directions()
    got, want = check(scene, terms, curved, horizontal)
    positive = terms[:, 3, None, None] > 0
    shadowed, blocked, lit = positive & ~want["go"], want["go"] & ~want["bits"], want["go"] & want["bits"]
    print(f"{shape[1]}x{shape[0]} curved={curved} horizontal={horizontal}: self-shadowed {int(shadowed.sum())}, blocked {int(blocked.sum())}, "
          f"lit {int(lit.sum())}")
    assert blocked.any() and lit.any(), "blocked and lit terms both occur"
    if horizontal:
        assert not shadowed.any() and np.array_equal(got["normal"], np.broadcast_to(f32([0, 1, 0]), got["normal"].shape))
    else:
        assert shadowed.any(), "self-shadowed terms occur: they are settled without a ray"
        length = np.linalg.norm(got["normal"].astype(np.float64), axis=-1)
        assert np.abs(length - 1.0).max() < 4e-7 and (got["normal"][..., 1] > 0).all()
    assert got["energy"].max() > 0 and int(got["count"].max()) <= 8
    if not horizontal and shape != (63, 65):  # the classes counted on the oracle when this was specified
        table = {(3, 5): (4, 4, 112), (33, 33): (1182, 458, 7072), (64, 64): (4116, 2498, 26154)}
        assert (int(shadowed.sum()), int(blocked.sum()), int(lit.sum())) == table[shape]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_direction_counts(irradiation_scenes, k):
    got, _ = check(irradiation_scenes[(63, 65)], directions(k), True)
    assert int(got["count"].max()) <= k
    if k == 3:
        check(irradiation_scenes[(33, 33)], directions(k), False, horizontal=True)


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65), (20, 20, 1, 1)])
def test_regions_are_windows_of_the_whole_raster(irradiation_scenes, region):
    scene = irradiation_scenes[(63, 65)]
    whole = contract_irradiation(scene, directions(), True)
    got, want = check(scene, directions(), True, region=region)
    r0, c0, r, c = region
    for key in ("energy", "count", "normal"):
        assert np.array_equal(want[key], whole[key][r0:r0 + r, c0:c0 + c]), key
    origins = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, region, 1e-3)
    assert same_bits(got["origins"], origins), "the visibility rasters' lifted lattice points"
    check(scene, directions(3), False, region=region, lift=0.5)


def test_normals_alone_need_no_direction(irradiation_scenes):
    scene = irradiation_scenes[(33, 33)]
    got = scene.irradiation(np.zeros((0, 4), f32))
    assert same_bits(got["normal"], contract_normals(contract_slope(scene, scene.region(None), False)))
    assert not got["energy"].any() and not got["count"].any()


def test_the_mesh_shades_and_terrain_only_ignores_it(irradiation_harness):
    import scenes

    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    scene = Scene(irradiation_harness, dem, _kw(dem, mesh_vertices=verts, mesh_indices=tris))
    try:
        terms = directions()
        full = scene.irradiation(terms, CURVED)
        bare = scene.irradiation(terms, CURVED | TERRAIN_ONLY)
        want = contract_irradiation(scene, terms, True)
        assert same_bits(bare["energy"], want["energy"]) and np.array_equal(bare["count"], want["count"]), "TERRAIN_ONLY: the oracle's terrain"
        assert (full["count"] <= bare["count"]).all() and (full["count"] < bare["count"]).any(), "the boxes only ever shade"
        assert same_bits(full["normal"], bare["normal"]), "the normals are the terrain's"
    finally:
        scene.close()


# ---- 2. no march for a term that is settled without a ray -----------------------------------------------------------------------
def test_settled_terms_never_march_and_add_nothing(irradiation_scenes):
    scene = irradiation_scenes[(63, 65)]
    good = directions(3)
    base = scene.irradiation(good, CURVED)
    for name, bad in (("zero weight", [0.3, 0.5, 0.2, 0.0]), ("negative weight", [0.3, 0.5, 0.2, -4.0]), ("NaN weight", [0.3, 0.5, 0.2, np.nan]),
                      ("NaN x", [np.nan, 0.5, 0.2, 9.0]), ("inf y", [0.3, np.inf, 0.2, 9.0]), ("-inf z", [0.3, 0.5, -np.inf, 9.0]),
                      ("zero direction", [0.0, 0.0, 0.0, 9.0]), ("straight down", [0.0, -1.0, 0.0, 9.0])):
        terms = np.concatenate([good[:2], np.array([bad], f32), good[2:]])
        got = scene.irradiation(terms, CURVED)
        assert not got["marches"][2].any(), name
        assert same_bits(got["energy"], base["energy"]) and np.array_equal(got["count"], base["count"]), f"{name}: adds nothing"
        assert np.array_equal(got["marches"][[0, 1, 3]], base["marches"]), name
    # a facet turned away: c <= 0 exactly where the march is skipped, on the slope and not on the horizontal plane
    low = np.array([sun_direction(90.0, 4.0)], f32)
    low[0, 3] = 5.0
    got, want = check(scene, low, True)
    away = ~want["go"][0]
    assert away.any() and (want["c"][0][away] <= 0).all() and not got["marches"][0][away].any()
    assert not got["energy"][away].any() and not got["count"][away].any()
    flat = scene.irradiation(low, CURVED | HORIZONTAL)
    assert (flat["marches"][0] >= 1).all(), "on a horizontal plane a sun above the horizontal always goes"


# ---- 3. an independent anchor: the planar incline ------------------------------------------------------------------------------
def test_planar_incline_against_the_analytic_normal(irradiation_harness):
    """h = 0.25 i + 0.5 j on 33 columns x 35 rows, spacing 1, exaggeration 1: every sample has the normal (-0.25, 1, -0.5) / |.|.  Of
    the 36 directions 26 have n.l >= 0.2 and no ray of theirs is blocked: for every sample the energy over them is sum wt (n.l),
    here in f64, within 64 x 2^-24 x sum wt -- under 16 roundings a term (each at most 2^-24 relative of a quantity bounded by
    wt), K <= 26 sequential adds (each at most 2^-24 of a partial sum bounded by sum wt): (16 + 26) 2^-24 sum wt < the bound.
    5 have n.l < 0 and contribute exactly 0 with no march.  Largest error met: 1.66e-4 Wh/m^2 = 1.26e-8 of sum wt (0.21 x 2^-24); the bound is 64 x 2^-24."""
    j, i = np.meshgrid(np.arange(35), np.arange(33), indexing="ij")
    dem = (0.25 * i + 0.5 * j).astype(f32)
    scene = Scene(irradiation_harness, dem, _planar(dem, 1.0))
    try:
        assert scene.spacing == (f32(1.0), f32(1.0)) and scene.kw["exaggeration"] == 1.0
        d = np.stack([sun_direction(az, el) for az in range(0, 360, 30) for el in (10, 35, 70)]).astype(f32)
        d[:, 3] = f32(50.0 + 25.0 * np.arange(36))
        n = np.array([-0.25, 1.0, -0.5]) / np.linalg.norm([-0.25, 1.0, -0.5])
        unit = d[:, :3].astype(np.float64)
        cosine = (unit @ n) / np.linalg.norm(unit, axis=1)
        high, away = cosine >= 0.2, cosine < 0.0
        assert int(high.sum()) == 26 and int(away.sum()) == 5
        assert contract_bits(scene, ALONG, d[high], False, None, 1e-3).all(), "the oracle blocks none of their rays"
        got = scene.irradiation(d[high])
        assert (got["count"] == 26).all()
        want = float((d[high, 3].astype(np.float64) * cosine[high]).sum())
        total = float(d[high, 3].astype(np.float64).sum())
        error = float(np.abs(got["energy"].astype(np.float64) - want).max())
        print(f"planar incline: largest error {error:.3e} = {error / total:.3e} of sum wt = {error / total * 2 ** 24:.2f} x 2^-24 (bound 64)")
        assert error <= 64.0 * 2.0 ** -24 * total
        assert np.abs(got["normal"].astype(np.float64) - n).max() <= 4.0 * 2.0 ** -24
        back = scene.irradiation(d[away])
        assert not back["energy"].any() and not back["count"].any() and not back["marches"].any(), "exactly 0, with no march"
    finally:
        scene.close()


# ---- 4. the interface -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_layout(irradiation_harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header, "the irradiation raster is additive: no ABI version bump"
    body = re.search(r"typedef struct f3d_session_irradiation_desc \{(.*?)\} f3d_session_irradiation_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [name for name, _ in _native.IrradiationDesc._fields_]
    assert members == ["struct_size", "flags", "row0", "col0", "rows", "cols", "lift", "direction_count", "directions", "energy", "count", "normal",
                       "reserved"]
    assert C.sizeof(_native.IrradiationDesc) == 72 == irradiation_harness.irradiation_desc_size()
    D = _native.IrradiationDesc
    assert D.lift.offset == 24 and D.directions.offset == 32 and D.normal.offset == 56 and D.reserved.offset == 64
    assert re.search(r"int f3d_session_irradiation\(f3d_session \*session, const f3d_session_irradiation_desc \*desc, char \*err, size_t errlen\);",
                     header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_irradiation"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for name, value in (("TERRAIN_ONLY", 1), ("CURVED", 2), ("DEVICE_POINTERS", 4), ("NO_WAIT", 8), ("HORIZONTAL", 16)):
        assert re.search(rf"#define F3D_IRRADIATION_{name} {value}u", header) and getattr(_native, f"IRRADIATION_{name}") == value
    assert (_native.IRRADIATION_TERRAIN_ONLY, _native.IRRADIATION_CURVED, _native.IRRADIATION_DEVICE_POINTERS, _native.IRRADIATION_NO_WAIT) == (
        _native.RASTER_TERRAIN_ONLY, _native.RASTER_CURVED, _native.RASTER_DEVICE_POINTERS, _native.RASTER_NO_WAIT), "the raster's flag values"


def test_wrapper_methods_and_argument_checks():
    from forge3d_amd.session import TerrainSession

    for name in ("irradiation", "surface_normals", "insolation", "irradiation_terms"):
        assert callable(getattr(TerrainSession, name))
    p = inspect.signature(TerrainSession.irradiation).parameters
    assert list(p)[1:3] == ["directions", "weights"] and p["weights"].default is None
    assert p["horizontal"].default is False and p["curved"].default is True and p["terrain_only"].default is False
    assert p["lift"].default == TerrainSession.SURFACE_BIAS and p["region"].default is None and p["count"].default is False and p["wait"].default is True
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("horizontal", "curved", "terrain_only", "lift", "region", "count", "wait"))
    p = inspect.signature(TerrainSession.surface_normals).parameters
    assert p["region"].default is None and p["wait"].default is True
    p = inspect.signature(TerrainSession.insolation).parameters
    assert p["dni"].default is None and p["dhi"].default is None and p["azimuths"].default == 16
    assert "slope" in TerrainSession.surface_normals.__doc__ and "aspect" in TerrainSession.surface_normals.__doc__
    assert "approximation" in TerrainSession.insolation.__doc__

    terms = TerrainSession.irradiation_terms
    d3 = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.5, -0.2, 0.5], [0.1, 0.3, 0.2]], np.float64)
    t = terms(d3, [1.0, 2.0, 3.0, 4.0])
    assert t.dtype == f32 and t.shape == (4, 4) and t.flags.c_contiguous
    assert np.array_equal(t[:, :3], d3.astype(f32)) and np.array_equal(t[:, 3], f32([1, 0, 0, 4])), "y <= 0: weight 0"
    assert np.array_equal(terms(np.concatenate([d3, [[1.0], [2.0], [3.0], [4.0]]], 1)), t), "(K, 4): the weight is the last column"
    assert terms(np.zeros((0, 3)), []).shape == (0, 4)
    for bad in (lambda: terms(d3), lambda: terms(d3, [1.0, 2.0]), lambda: terms(t, [1.0] * 4), lambda: terms(np.zeros((3, 2)), [1.0] * 3),
                lambda: terms(np.zeros(3), [1.0])):
        with pytest.raises(ValueError):
            bad()


# ---- 5. sun_track and clear_sky -------------------------------------------------------------------------------------------------
def test_sun_track_is_the_ephemeris_at_the_step_midpoints():
    where = dict(lat=46.85, lon=-121.76)
    track = insolation.sun_track((2024, 6, 21), **where, step_minutes=30, tz_offset_hours=-8.0, elev_m=1600.0, pressure_mbar=840.0)
    d, el, hours, utc = track["directions"], track["elevation_deg"], track["hours"], track["utc"]
    assert d.dtype == f32 and d.shape == (len(utc), 3) and el.shape == hours.shape == (len(utc),)
    assert 28 <= len(utc) <= 34, "near sixteen hours of daylight at the solstice"
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 2e-7, "unit to f32"
    assert (d[:, 1] > 0).all() and (el > 0).all()
    every = [(2024, 6, 21, k // 2, 15 + 30 * (k % 2), 0.0) for k in range(48)]
    suns = [geo.solar_position(u, where["lat"], where["lon"], 1600.0, tz_offset_hours=-8.0, pressure_mbar=840.0) for u in every]
    up = [k for k in range(48) if suns[k]["apparent_elevation_deg"] > 0.0]
    assert utc == [every[k] for k in up], "the step midpoints of the civil day, those above the horizon"
    for row, e, k in zip(d, el, up):
        az_r, el_r = np.radians(suns[k]["azimuth_deg"]), np.radians(suns[k]["apparent_elevation_deg"])
        want = np.array([np.sin(az_r) * np.cos(el_r), np.sin(el_r), -np.cos(az_r) * np.cos(el_r)]).astype(f32)
        assert np.array_equal(row, want) and e == suns[k]["apparent_elevation_deg"]
    assert np.array_equal(hours, np.full(len(up), 0.5)) and hours.sum() == 0.5 * len(up), "hours sum to the daylight steps"
    noon = int(np.argmax(el))
    assert d[noon, 2] > 0 and abs(d[noon, 0]) < 0.2, "at noon the sun stands in the south (+z) at this latitude"
    # a step that does not divide the day: the last one is shorter; a date object; a polar night
    import datetime

    odd = insolation.sun_track(datetime.date(2024, 6, 21), 0.0, 0.0, step_minutes=420)
    assert len(odd["utc"]) <= 4 and set(odd["hours"]) <= {7.0, 3.0}
    night = insolation.sun_track((2024, 12, 21), 80.0, 0.0)
    assert night["directions"].shape == (0, 3) and night["hours"].shape == (0,) and night["utc"] == []
    with pytest.raises(ValueError):
        insolation.sun_track((2024, 6, 21), 0.0, 0.0, step_minutes=0)


def test_clear_sky_is_the_two_formulas():
    el = np.array([-5.0, 0.0, 0.01, 1.0, 5.0, 15.0, 30.0, 45.0, 60.0, 89.0, 90.0])
    for altitude in (0.0, 1600.0, 4392.0):
        dni, dhi = insolation.clear_sky(el, altitude)
        assert dni.dtype == np.float64 and dni.shape == el.shape
        a = altitude / 1000.0
        for e, got_n, got_h in zip(el, dni, dhi):
            if e <= 0.0:
                assert got_n == 0.0 and got_h == 0.0
                continue
            am = 1.0 / (np.sin(np.radians(e)) + 0.50572 * (e + 6.07995) ** -1.6364)
            want = 1353.0 * ((1.0 - 0.14 * a) * 0.7 ** (am ** 0.678) + 0.14 * a)
            assert abs(got_n - want) <= 1e-12 * want and abs(got_h - 0.1 * want) <= 1e-12 * want
        assert (np.diff(dni[1:]) > 0).all(), "monotone in elevation"
    sea, high = insolation.clear_sky(30.0)[0], insolation.clear_sky(30.0, 3000.0)[0]
    assert 700.0 < float(sea) < 850.0 and float(high) > float(sea)
    assert float(insolation.clear_sky(0.0)[0]) == 0.0 and np.ndim(insolation.clear_sky(10.0)[0]) == 0
    assert "rule of thumb" in insolation.clear_sky.__doc__.lower()


# ---- 6. the sanitizer run: a stand-alone program, never code loaded into this process -------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(HARNESS, "irradiation")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "terms that broke the contract: 0" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
