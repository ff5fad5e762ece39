"""Horizon rasters on a live terrain session (f3d_session_horizon), the parts that need no GPU.

The lane body of the horizon kernel (csrc/f3d_horizon.h horizon_lane, what k_horizon calls per lane) compiled for the host
(tests/horizon_host) and run over the kernel's waves and lanes (csrc/f3d_walk.h region_sample), against
tests/horizon_reference.py -- an independent float64 statement of the contract that cuts the line at every lattice line and
knows nothing of the pyramid or the walk.

* DEMs 5x3, 33x33, 64x64 and 65x63 (test_session_raster_host.SHAPES, its spacing and exaggeration); K = 16 compass azimuths
  (the axis-aligned headings run along cell edges, the 45-degree ones through corners where the cells are square), K = 1 and
  K = 3 with directions that are not normalised (one axis-aligned, one nearly so), lifts 1e-3 and 0.5, curved and flat;
* -inf exactly where the reference has it, no NaN, elsewhere |H - H64| <= TOL (1 + |H64|).  TOL is 8 x the largest such ratio
  MEASURED over exactly these inputs (2.34e-6, 64x64, K = 1, lift 0.5, curved): see MEASURED below and DESIGN.md;
* planes with a known answer (a planar DEM, a flat one), sky_view against the stated formula in NumPy float32 bit for bit,
  regions, both wave footprints, the step cap (injected here only), the reference itself against dense sampling, and the
  share of samples the GPU suite's bracket test has to leave out, on the reference;
* a stand-alone driver (its own main) of the same lane body built with -fsanitize=address,undefined and run once;
* the header, the ctypes table and the descriptor's layout; the wrapper's methods.
The refusals of f3d_session_horizon need a session, i.e. a device: tests/test_gpu_horizon.py.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import horizon_reference as ref
import scenes
from emul import emul
from test_session_raster_host import SHAPES, _kw, _planar, contract_origins, shaped_dem
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "horizon_host" / "horizon_harness.cpp"
SIZE = (96, 64)
CURVED = 2
f32 = np.float32

# The largest |H - H64| / (1 + |H64|) of the host body against the float64 reference over AZIMUTH_SETS x LIFTS x curved / flat
# x SHAPES, measured (test_host_body_against_the_reference prints each case's); the bound is 8 x it.  10 x TOL = 1.9e-4 stays
# below the 1e-3 band the GPU suite's bracket test leaves out.
MEASURED = 2.34e-6
TOL = 8.0 * MEASURED
LIFTS = (1e-3, 0.5)
SLOPES = (-0.2, 0.0, 0.1, 0.25, 0.5)  # the bracket test's (tests/test_gpu_horizon.py)


def compass(n=16):
    from forge3d_amd.session import TerrainSession

    return TerrainSession.horizon_directions(n)


AZIMUTH_SETS = {"compass16": None, "one": np.array([[3.0, -1.5]], f32), "three": np.array([[-0.7, 2.2], [0.0, -4.0], [1e-3, 5e-4]], f32)}


def azimuth_set(name):
    return compass(16) if name == "compass16" else AZIMUTH_SETS[name]


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "horizon_host")
    lib.horizon_scene_create.restype = C.c_void_p
    lib.horizon_scene_create.argtypes = [C.c_void_p, C.c_void_p]
    lib.horizon_scene_destroy.argtypes = [C.c_void_p]
    lib.horizon_run.restype = C.c_int
    lib.horizon_run.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_float, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] * 2
    lib.horizon_step_cap_of.restype = C.c_uint32
    lib.horizon_step_cap_of.argtypes = [C.c_void_p]
    lib.horizon_desc_size.restype = C.c_uint32
    return lib


class HostScene:
    """A scene as the emulator sets it up, and horizon rasters over it as f3d_session_horizon's device form answers them."""

    def __init__(self, lib, dem, kw):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        d, keep = _desc(self.dem, SIZE, scenes.CAM, kw)
        info = np.zeros(6, f32)
        self.handle = lib.horizon_scene_create(C.addressof(d), info.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin, self.spacing = (f32(info[0]), f32(info[1])), (f32(info[2]), f32(info[3]))
        self.inv_two_r_prime, self.curvature_enabled = f32(info[4]), bool(info[5])
        self.surface = ref.Surface(self.dem, kw["exaggeration"], self.origin, self.spacing)
        self.step_cap = int(lib.horizon_step_cap_of(self.handle))
        self._reference = {}

    def close(self):
        self.lib.horizon_scene_destroy(self.handle)

    def region(self, region):
        return (0, 0, *self.dem.shape) if region is None else tuple(int(v) for v in region)

    def run(self, azimuths, lift, curved=False, region=None, planes=True, sky=True, cap=0, block=0):
        row0, col0, rows, cols = self.region(region)
        az = np.ascontiguousarray(azimuths, f32).reshape(-1, 2)
        k, n = len(az), rows * cols
        h = np.full((k, n), 77.0, f32) if planes else None
        s = np.full(n, 77.0, f32) if sky else None
        o = np.full((n, 3), 77.0, f32)
        assert self.lib.horizon_run(self.handle, CURVED if curved else 0, row0, col0, rows, cols, float(lift), k, az.ctypes.data,
                                    h.ctypes.data if planes else None, s.ctypes.data if sky else None, o.ctypes.data, cap, block) == 0
        return {"horizon": h.reshape(k, rows, cols) if planes else None, "sky_view": s.reshape(rows, cols) if sky else None,
                "origins": o.reshape(rows, cols, 3)}

    def reference(self, name, lift, curved):
        """The float64 planes of a named azimuth set over the whole DEM: computed once, shared, never written to."""
        key = (name, float(lift), bool(curved))
        if key not in self._reference:
            got = ref.horizon_reference(self.surface, self.region(None), lift, azimuth_set(name), self.inv_two_r_prime,
                                        curved and self.curvature_enabled)
            got.setflags(write=False)
            self._reference[key] = got
        return self._reference[key]


@pytest.fixture(scope="module")
def shaped(harness):
    made = {}
    for shape in SHAPES:
        dem = shaped_dem(shape)
        made[shape] = HostScene(harness, dem, _kw(dem))
    yield made
    for s in made.values():
        s.close()


def compare(got, want, tol=TOL):
    """-inf where the reference has it, no NaN, elsewhere the relative bound; returns the largest ratio."""
    assert not np.isnan(got).any(), "no NaN"
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), "-inf exactly where the reference has -inf"
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    ratio = np.abs(got[fin].astype(np.float64) - want[fin]) / (1.0 + np.abs(want[fin]))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= tol, f"|H - H64| / (1 + |H64|) reaches {worst:.3g}, the bound is {tol:.3g}"
    return worst


# ---- the host body against the float64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_host_body_against_the_reference(shaped, shape, curved):
    scene = shaped[shape]
    assert scene.curvature_enabled and scene.inv_two_r_prime > 0.0
    for name in AZIMUTH_SETS:
        for lift in LIFTS:
            got = scene.run(azimuth_set(name), lift, curved)
            worst = compare(got["horizon"], scene.reference(name, lift, curved))
            print(f"{shape[1]}x{shape[0]} {name} lift {lift} {'curved' if curved else 'flat'}: largest ratio {worst:.3g} (bound {TOL:.3g})")
            want_o = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, scene.region(None), lift)
            assert np.array_equal(got["origins"].view(np.uint32), want_o.view(np.uint32)), "the rasters' lifted lattice points"
    if shape[0] * shape[1] > 64:
        h = scene.reference("compass16", 1e-3, curved)
        assert np.isneginf(h).any() and (h[np.isfinite(h)] > 0).any() and (h[np.isfinite(h)] < 0).any()


def test_curvature_lowers_the_horizon_by_the_k_term(shaped):
    """Curved and flat differ, by the reference's k term: on a far horizon at parameter t the drop is k t."""
    scene = shaped[(63, 65)]
    az = azimuth_set("one")
    flat, curved = scene.run(az, 0.5, False)["horizon"], scene.run(az, 0.5, True)["horizon"]
    fin = np.isfinite(flat)
    assert (curved[fin] <= flat[fin]).all() and (curved[fin] < flat[fin]).any()
    k = ref.curvature_k(az[0], scene.inv_two_r_prime, True)
    t_exit = ref.horizon_reference(scene.surface, scene.region(None), 0.5, az, return_exit=True)[1]
    assert (flat[fin].astype(np.float64) - curved[fin] <= k * t_exit[fin] * (1 + 1e-3) + 2 * TOL * (1 + np.abs(flat[fin]))).all()


def test_lift_zero_includes_the_directional_derivative(shaped):
    scene = shaped[(33, 33)]
    got = scene.run(compass(16), 0.0)["horizon"]
    want = ref.horizon_reference(scene.surface, scene.region(None), 0.0, compass(16))
    compare(got, want)
    lifted = scene.reference("compass16", 1e-3, False)
    fin = np.isfinite(want)
    assert (want[fin] >= lifted[fin]).all(), "a lower eye has a higher horizon"


def test_reference_against_dense_sampling(shaped):
    """The reference's closed form per segment against brute force: 4000 parameters a cell along the line."""
    for shape, samples in (((3, 5), [(0, 0), (1, 2), (2, 4), (1, 0)]), ((33, 33), [(16, 16), (3, 30), (32, 0)])):
        scene = shaped[shape]
        for name in AZIMUTH_SETS:
            az = azimuth_set(name)
            want = scene.reference(name, 1e-3, False)
            for j, i in samples:
                for k in range(0, len(az), 3):
                    dense = ref.dense_horizon(scene.surface, (j, i), 1e-3, az[k])
                    if np.isneginf(want[k, j, i]):
                        assert np.isneginf(dense)
                    else:  # (sampling can only fall short of the supremum, by its step)
                        assert -1e-5 * (1 + abs(dense)) <= want[k, j, i] - dense <= 1e-4 * (1 + abs(dense)), (shape, name, j, i, k)


# ---- inputs with known answers -----------------------------------------------------------------------------------------------
def planar_scene(harness, a, b, shape=(17, 21)):
    rows, cols = shape
    x = (np.arange(cols, dtype=np.float64) - 0.5 * (cols - 1))[None, :]
    z = (np.arange(rows, dtype=np.float64) - 0.5 * (rows - 1))[:, None]
    dem = (a * x + b * z).astype(f32)  # (spacing 1, origin -(n - 1) / 2: multiples of 1 / 8, exact in float32)
    assert np.array_equal(dem.astype(np.float64), a * x + b * z)
    return HostScene(harness, dem, _planar(dem, 1.0))


def test_planar_dem(harness):
    """y = a x + b z: H = a dx + b dz on every sample with terrain ahead (lift 0: the directional derivative, also where it
    is the limit t -> 0+); lifted, H = a dx + b dz - lift / t_exit, reached where the line leaves the footprint."""
    a, b = 0.25, -0.5
    scene = planar_scene(harness, a, b)
    try:
        for az in (compass(16), azimuth_set("one"), azimuth_set("three")):
            slope = (a * az[:, 0].astype(np.float64) + b * az[:, 1].astype(np.float64))[:, None, None]
            t_exit = ref.horizon_reference(scene.surface, scene.region(None), 0.0, az, return_exit=True)[1]
            ahead = t_exit > 0.0
            for lift in (0.0, 0.5):
                got = scene.run(az, lift)["horizon"]
                with np.errstate(divide="ignore"):
                    want = np.where(ahead, slope - (np.float64(f32(lift)) / t_exit if lift else 0.0), -np.inf)
                compare(got, want)
            assert ahead.any() and not ahead.all()
    finally:
        scene.close()


def test_flat_dem_has_sky_view_one(harness):
    dem = np.full((9, 12), 3.5, f32)
    scene = HostScene(harness, dem, _planar(dem, 2.0))
    try:
        for lift in (0.0, 1e-3, 0.5):
            for curved in (False, True):
                got = scene.run(compass(16), lift, curved)
                assert (got["sky_view"] == f32(1.0)).all(), "exactly 1"
                assert (got["horizon"] <= 0.0).all()
    finally:
        scene.close()


def test_sky_view_is_one_wherever_no_horizon_is_positive(shaped):
    scene = shaped[(63, 65)]
    got = scene.run(compass(16), 0.5)
    low = (got["horizon"] <= 0.0).all(axis=0)
    assert low.any() and (got["sky_view"][low] == f32(1.0)).all()
    assert (got["sky_view"][~low] < f32(1.0)).all() and (got["sky_view"] > 0.0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_sky_view_is_the_stated_formula_bit_for_bit(shaped, shape):
    scene = shaped[shape]
    for name in AZIMUTH_SETS:
        az = azimuth_set(name)
        for curved in (False, True):
            both = scene.run(az, 1e-3, curved)
            want = ref.sky_view_f32(both["horizon"], az)
            assert np.array_equal(both["sky_view"].view(np.uint32), want.view(np.uint32))
            alone = scene.run(az, 1e-3, curved, planes=False)
            assert alone["horizon"] is None and np.array_equal(alone["sky_view"].view(np.uint32), want.view(np.uint32)), "with horizon null as well"
            planes_only = scene.run(az, 1e-3, curved, sky=False)
            assert np.array_equal(planes_only["horizon"].view(np.uint32), both["horizon"].view(np.uint32))


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65), (20, 20, 1, 1)])
def test_regions(shaped, region):
    scene = shaped[(63, 65)]
    az = compass(16)
    whole = scene.run(az, 0.5, True)
    r0, c0, r, c = region
    for block in (0, 1):
        got = scene.run(az, 0.5, True, region=region, block=block)
        assert np.array_equal(got["horizon"].view(np.uint32), whole["horizon"][:, r0:r0 + r, c0:c0 + c].view(np.uint32)), "a window of the whole raster"
        assert np.array_equal(got["sky_view"].view(np.uint32), whole["sky_view"][r0:r0 + r, c0:c0 + c].view(np.uint32))
    compare(got["horizon"], scene.reference("compass16", 0.5, True)[:, r0:r0 + r, c0:c0 + c])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_both_wave_footprints_give_the_same_bits(shaped, shape):
    scene = shaped[shape]
    az = azimuth_set("three")
    row, block = scene.run(az, 1e-3, block=0), scene.run(az, 1e-3, block=1)
    assert np.array_equal(row["horizon"].view(np.uint32), block["horizon"].view(np.uint32))
    assert np.array_equal(row["sky_view"].view(np.uint32), block["sky_view"].view(np.uint32))
    assert not (block["horizon"] == 77.0).any() and not (block["sky_view"] == 77.0).any(), "every sample is written"


def test_step_cap(shaped):
    """An injected tiny cap (the harness alone can): a lane whose walk is not over after `cap` steps writes qNaN for that
    azimuth and goes on to the next; its sky-view sum takes 0 from it.  The real cap is never reached."""
    scene = shaped[(63, 65)]
    az = compass(16)
    full = scene.run(az, 1e-3)
    assert not np.isnan(full["horizon"]).any() and scene.step_cap == 4 * (64 + 62) + 8 * 7
    capped = scene.run(az, 1e-3, cap=3)
    nan = np.isnan(capped["horizon"])
    assert nan.any() and not nan.all()
    assert (capped["horizon"].view(np.uint32)[nan] == 0x7FC00000).all(), "the quiet NaN"
    assert np.array_equal(capped["horizon"][~nan].view(np.uint32), full["horizon"][~nan].view(np.uint32)), "a walk that ends within the cap is untouched"
    assert nan[1].any() and (~nan[1]).any(), "per azimuth: a lane goes on after a capped one"
    want = ref.sky_view_f32(capped["horizon"], az)
    assert np.array_equal(capped["sky_view"].view(np.uint32), want.view(np.uint32)) and not np.isnan(capped["sky_view"]).any()


def test_nan_azimuths_answer_nan(shaped):
    """The device form's path: the host never sees the azimuths, the lanes answer a non-finite or zero one with NaN."""
    scene = shaped[(33, 33)]
    good = azimuth_set("one")[0]
    for bad in ([np.nan, 1.0], [1.0, np.inf], [-np.inf, 0.0], [0.0, 0.0]):
        az = np.array([good, bad, good], f32)
        got = scene.run(az, 1e-3)
        assert np.isnan(got["horizon"][1]).all() and not np.isnan(got["horizon"][[0, 2]]).any()
        assert np.array_equal(got["horizon"][0].view(np.uint32), got["horizon"][2].view(np.uint32))
        with np.errstate(all="ignore"):
            assert np.array_equal(got["sky_view"].view(np.uint32), ref.sky_view_f32(got["horizon"], az).view(np.uint32))


# ---- the bracket the GPU suite checks against visibility(), on the reference --------------------------------------------------
def left_out(h, slope):
    with np.errstate(invalid="ignore"):
        return np.isfinite(h) & (np.abs(slope - h) <= 1e-3 * (1.0 + np.abs(h)))


def test_bracket_leaves_out_at_most_two_percent(shaped):
    """tests/test_gpu_horizon.py compares `slope > H` with visibility() wherever |slope - H| > 1e-3 (1 + |H|): the share of
    samples left out, on the float64 reference, per slope and over all 16 compass azimuths."""
    for shape in ((33, 33), (63, 65)):
        h = shaped[shape].reference("compass16", 1e-3, False)
        shares = [float(left_out(h, s).mean()) for s in SLOPES]
        lit = [float((s > h).mean()) for s in SLOPES]
        print(f"{shape[1]}x{shape[0]}: left out " + " / ".join(f"{100 * v:.2f} %" for v in shares) + "; lit " + " / ".join(f"{v:.3f}" for v in lit))
        assert max(shares) <= 0.02
        assert lit[0] < 0.2 and lit[-1] > 0.8 and all(x < y for x, y in zip(lit, lit[1:])), "the slopes cut through the distribution"


# ---- the samples a wave owns: csrc/f3d_walk.h region_sample over region_waves, what the three kernels are launched with --------
def test_region_sample_hands_out_every_sample_exactly_once(harness):
    harness.horizon_region_counts.restype = C.c_uint32
    harness.horizon_region_counts.argtypes = [C.c_uint32] * 3 + [C.c_void_p]
    for rows, cols in ((1, 1), (1, 65), (65, 1), (7, 9), (8, 8), (9, 17), (63, 65)):
        for block in (0, 1):
            counts = np.zeros(rows * cols, np.uint32)
            outside = harness.horizon_region_counts(rows, cols, block, counts.ctypes.data)
            assert outside == 0 and (counts == 1).all(), (rows, cols, block, outside, np.flatnonzero(counts != 1)[:8])


# ---- the sanitizer run: a stand-alone program, never code loaded into this process ---------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(HARNESS, "horizon")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "NaN without an injected cap: 0" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header, "the horizon raster is additive: no ABI version bump"
    body = re.search(r"typedef struct f3d_session_horizon_desc \{(.*?)\} f3d_session_horizon_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [name for name, _ in _native.HorizonDesc._fields_]
    assert members == ["struct_size", "flags", "row0", "col0", "rows", "cols", "lift", "azimuth_count", "azimuths", "horizon", "sky_view", "reserved"]
    assert C.sizeof(_native.HorizonDesc) == 64 == harness.horizon_desc_size()
    assert _native.HorizonDesc.lift.offset == 24 and _native.HorizonDesc.azimuths.offset == 32 and _native.HorizonDesc.reserved.offset == 56
    assert re.search(r"int f3d_session_horizon\(f3d_session \*session, const f3d_session_horizon_desc \*desc, char \*err, size_t errlen\);", header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_horizon"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for name, value in (("CURVED", 2), ("DEVICE_POINTERS", 4), ("NO_WAIT", 8), ("MAX_AZIMUTHS", 256)):
        assert re.search(rf"#define F3D_HORIZON_{name} {value}u", header) and getattr(_native, f"HORIZON_{name}") == value
    assert _native.HORIZON_CURVED == _native.RASTER_CURVED and _native.HORIZON_DEVICE_POINTERS == _native.RASTER_DEVICE_POINTERS
    assert _native.HORIZON_NO_WAIT == _native.RASTER_NO_WAIT, "the raster's flag values"


def test_wrapper_has_the_horizon_methods():
    import inspect

    from forge3d_amd.session import TerrainSession

    for name in ("horizon", "sky_view_factor", "horizon_directions"):
        assert callable(getattr(TerrainSession, name))
    p = inspect.signature(TerrainSession.horizon).parameters
    assert p["azimuths"].default == 16 and p["lift"].default == TerrainSession.SURFACE_BIAS and p["curved"].default is False
    assert p["region"].default is None and p["sky_view"].default is False and p["wait"].default is True
    assert "sky_view" not in inspect.signature(TerrainSession.sky_view_factor).parameters
    d = TerrainSession.horizon_directions(16)
    assert d.dtype == f32 and d.shape == (16, 2)
    a = np.radians(360.0 * np.arange(16) / 16)
    assert np.array_equal(d, np.stack([np.sin(a), -np.cos(a)], 1).astype(f32)), "(sin a, -cos a): sun_azimuth_deg's convention"
    assert np.array_equal(d[0], f32([0.0, -1.0])) and d[4, 0] == 1.0 and abs(d[4, 1]) < 1e-7
    given = np.array([[3.0, -1.5], [0.0, 2.0]], np.float64)
    assert np.array_equal(TerrainSession.horizon_directions(given), given.astype(f32))
    for bad in (0, 257):
        with pytest.raises(ValueError):
            TerrainSession.horizon_directions(bad)
    with pytest.raises(ValueError):
        TerrainSession.horizon_directions(np.zeros((3, 3), f32))
