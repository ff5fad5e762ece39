"""Shadow-depth rasters on a live terrain session (f3d_session_umbra), the parts that need no GPU.

The lane body of the umbra kernel (csrc/f3d_umbra.h umbra_sample / umbra_depth, what k_umbra runs per lane) compiled for the host
(tests/umbra_host) and run over the kernel's waves and lanes (csrc/f3d_walk.h region_sample), against tests/umbra_reference.py -- an independent
float64 statement of the contract that cuts the line at every lattice line and knows nothing of the pyramid or the walk.

* DEMs 5x3, 33x33, 64x64 and 65x63 (test_session_raster_host.SHAPES, its spacing and exaggeration), curved and flat; ten
  directions (`directions` below): the sun at azimuth 315 and elevation 5 / 15 / 30, along +x, along -z, the cell diagonal
  (through lattice corners), level (dy = 0), descending (dy = -0.05), straight up and straight down;
* +inf, exact +0 and qNaN exactly where the reference and the contract have them, every value >= 0, elsewhere
  |L - L64| <= TOL (1 + |L64| + |h| + relief) -- the rounding floor is an ulp of the heights, not of L.  TOL is 8 x the largest
  such ratio MEASURED over exactly these inputs: see MEASURED below and DESIGN.md;
* inputs with known answers (a planar DEM tilted toward and away from the direction, the raster tests' ridge, the earth's bulge
  over a flat DEM), regions, both wave footprints, the step cap (injected here only), bad directions, `deepest`, the session's
  sun, the reference itself against dense sampling, the horizon raster's host body as a second opinion on lit / shadowed, and
  the share of samples the GPU suite's bracket test has to leave out, on the reference;
* a stand-alone driver (its own main) of the same lane body built with -fsanitize=address,undefined and run once;
* the header, the ctypes table, the descriptor's layout and INTEGRATION.md's struct; the wrapper's methods.
The refusals of f3d_session_umbra need a session, i.e. a device: tests/test_gpu_umbra.py.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scenes
import umbra_reference as ref
from emul import emul
from test_session_raster_host import SHAPES, _kw, _planar, contract_origins, shaped_dem, sun_direction
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "umbra_host" / "umbra_harness.cpp"
SIZE = (96, 64)
CURVED, SESSION_SUN = 2, 16
f32 = np.float32

# The largest |L - L64| / (1 + |L64| + |h| + relief) of the host body against the float64 reference over the ten directions x
# curved / flat x SHAPES, measured (test_host_body_against_the_reference prints each case's: 65x63, curved, the sun at elevation 5);
# the bound is 8 x it -- the margin the clearance tests use: the measured maximum is one draw of a rounding error whose worst case
# over other inputs is a small multiple of it.  10 x TOL stays below the 2e-3 band the GPU suite's bracket leaves out.
MEASURED = 2.01e-6
TOL = 8.0 * MEASURED
RUNGS = (0.25, 1.0, 3.0, 8.0)  # the bracket test's lifts (tests/test_gpu_umbra.py)
BAND = 2e-3


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "umbra_host")
    lib.umbra_scene_create.restype = C.c_void_p
    lib.umbra_scene_create.argtypes = [C.c_void_p, C.c_void_p]
    lib.umbra_scene_destroy.argtypes = [C.c_void_p]
    lib.umbra_run.restype = C.c_int
    lib.umbra_run.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 4 + [C.c_uint32] * 2
    lib.umbra_horizon_run.restype = C.c_int
    lib.umbra_horizon_run.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.umbra_step_cap_of.restype = C.c_uint32
    lib.umbra_step_cap_of.argtypes = [C.c_void_p]
    lib.umbra_desc_size.restype = C.c_uint32
    return lib


class HostScene:
    """A scene as the emulator sets it up, and shadow-depth rasters over it as f3d_session_umbra's device form answers them."""

    def __init__(self, lib, dem, kw, cam=None):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        d, keep = _desc(self.dem, SIZE, cam or scenes.CAM, kw)
        info = np.zeros(9, f32)
        self.handle = lib.umbra_scene_create(C.addressof(d), info.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin, self.spacing = (f32(info[0]), f32(info[1])), (f32(info[2]), f32(info[3]))
        self.inv_two_r_prime, self.curvature_enabled = f32(info[4]), bool(info[5])
        self.sun = info[6:9].copy()
        self.surface = ref.Surface(self.dem, kw["exaggeration"], self.origin, self.spacing)
        self.relief = float(self.surface.h64.max() - self.surface.h64.min())
        self.step_cap = int(lib.umbra_step_cap_of(self.handle))
        self._reference = {}

    def close(self):
        self.lib.umbra_scene_destroy(self.handle)

    def region(self, region):
        return (0, 0, *self.dem.shape) if region is None else tuple(int(v) for v in region)

    def run(self, directions, curved=False, region=None, planes=True, deepest=True, cap=0, block=0):
        """directions None: the session's sun (SESSION_SUN)."""
        row0, col0, rows, cols = self.region(region)
        if directions is None:
            flags, k, ptr = SESSION_SUN, 1, None
        else:
            d = np.ascontiguousarray(directions, f32).reshape(-1, 4)
            flags, k, ptr = 0, len(d), d.ctypes.data
        n = rows * cols
        p = np.full((k, n), 77.0, f32) if planes else None
        deep = np.full(n, 77.0, f32) if deepest else None
        g = np.full((n, 3), 77.0, f32)
        assert self.lib.umbra_run(self.handle, flags | (CURVED if curved else 0), row0, col0, rows, cols, k, ptr, p.ctypes.data if planes else None,
                                  deep.ctypes.data if deepest else None, g.ctypes.data, cap, block) == 0
        return {"depth": p.reshape(k, rows, cols) if planes else None, "deepest": deep.reshape(rows, cols) if deepest else None,
                "samples": g.reshape(rows, cols, 3)}

    def horizon(self, azimuths, curved=False, lift=0.0):
        az = np.ascontiguousarray(azimuths, f32).reshape(-1, 2)
        out = np.full((len(az), *self.dem.shape), 77.0, f32)
        assert self.lib.umbra_horizon_run(self.handle, CURVED if curved else 0, float(lift), len(az), az.ctypes.data, out.ctypes.data) == 0
        return out

    def reference(self, direction, curved):
        """(L64, along) of one direction over the whole DEM: computed once, shared, never written to."""
        key = (np.asarray(direction, f32).tobytes(), bool(curved))
        if key not in self._reference:
            got = ref.umbra_reference(self.surface, self.region(None), direction, self.inv_two_r_prime, curved and self.curvature_enabled,
                                      return_along=True)
            for a in got:
                a.setflags(write=False)
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


NAMES = ("sun 315 / 5", "sun 315 / 15", "sun 315 / 30", "along +x", "along -z", "the cell diagonal", "level", "descending", "straight up",
         "straight down")
WALKED = 8  # the first eight take a walk; the last two are special values


def directions(scene):
    """The ten directions of the module's docstring, (10, 4) float32, in the order of NAMES."""
    sx, sz = float(scene.spacing[0]), float(scene.spacing[1])
    return np.array([sun_direction(315.0, 5.0), sun_direction(315.0, 15.0), sun_direction(315.0, 30.0),
                     [1.0, 0.17, 0.0, 0.0], [0.0, 0.34, -1.0, 0.0], [sx, 0.2, sz, 0.0],
                     [-0.8, 0.0, 0.6, 0.0], [0.6, -0.05, 0.8, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0]], f32)


def compare(got, want, along, h, relief, tol=None):
    """+inf and NaN where the reference has them, exactly +0 without terrain along the direction, every value >= 0, elsewhere the
    bound; returns the largest ratio."""
    tol = TOL if tol is None else tol
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN exactly where the contract has NaN"
    assert (got.view(np.uint32)[np.isnan(got)] == 0x7FC00000).all(), "the quiet NaN"
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), "+inf exactly where the reference has +inf"
    fin = np.isfinite(want)
    assert (got[fin] >= 0).all() and not np.signbit(got[fin]).any(), "every value >= +0"
    none = ~along & fin
    assert (got[none].view(np.uint32) == 0).all() and (want[none] == 0.0).all(), "exactly +0 where no terrain lies along the direction"
    assert (got[fin & (want == 0.0) & (got == 0.0)].view(np.uint32) == 0).all()
    ratio = np.abs(got[fin].astype(np.float64) - want[fin]) / (1.0 + np.abs(want[fin]) + np.abs(h[fin]) + relief)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= tol, f"|L - L64| / (1 + |L64| + |h| + relief) reaches {worst:.3g}, the bound is {tol:.3g}"
    return worst


# ---- the host body against the float64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_host_body_against_the_reference(shaped, shape, curved):
    scene = shaped[shape]
    assert scene.curvature_enabled and scene.inv_two_r_prime > 0.0
    dirs = directions(scene)
    got = scene.run(dirs, curved)
    want_g = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, scene.region(None), 0.0)
    assert np.array_equal(got["samples"].view(np.uint32), want_g.view(np.uint32)), "the rasters' lattice points, lift 0"
    h = scene.surface.h64
    for k, name in enumerate(NAMES):
        want, along = scene.reference(dirs[k], curved)
        worst = compare(got["depth"][k], want, along, h, scene.relief)
        print(f"{shape[1]}x{shape[0]} {'curved' if curved else 'flat'} {name}: largest ratio {worst:.3g} (bound {TOL:.3g}), "
              f"{int((want == 0).sum())} zero, {int((want > 0).sum())} in shadow of {want.size}, deepest {float(want.max()):.4g}")
    assert (got["depth"][8].view(np.uint32) == 0).all(), "straight up: +0 everywhere, no walk"
    assert np.isposinf(got["depth"][9]).all(), "straight down: +inf everywhere, no walk"
    rows, cols = scene.dem.shape
    if rows * cols > 64:
        for k in range(WALKED):  # (both answers occur; the 33x33 crop's coarser cells leave nothing in shadow at elevation 30)
            assert (got["depth"][k] == 0).any() and ((got["depth"][k] > 0).any() or (k == 2 and rows == 33)), NAMES[k]
    # along +x the last row has no cell beside it, along -z the last column: the contract's footprint
    assert (got["depth"][3][-1] == 0).all() and (got["depth"][4][:, -1] == 0).all()
    assert (got["depth"][3][:, -1] == 0).all() and (got["depth"][4][0] == 0).all(), "border samples looking outward"


def test_a_lower_sun_casts_a_deeper_shadow(shaped):
    scene = shaped[(63, 65)]
    d = scene.run(directions(scene)[:3], True)["depth"]
    slack = TOL * (1 + np.abs(d[0]) + np.abs(scene.surface.h64) + scene.relief)
    assert (d[0] >= d[1] - slack).all() and (d[1] >= d[2] - slack).all(), "same azimuth: the depth falls as the sun rises"
    assert d[0].max() > d[2].max() > 0


def test_reference_against_dense_sampling(shaped):
    """The reference's closed form per segment against brute force: 4000 parameters a cell along the line."""
    for shape, samples in (((3, 5), [(0, 0), (1, 2), (2, 4), (1, 0)]), ((33, 33), [(16, 16), (3, 30), (32, 0), (0, 32), (20, 7), (31, 31)])):
        scene = shaped[shape]
        dirs = directions(scene)
        for k in range(WALKED):
            for curved in (False, True):
                want, _ = scene.reference(dirs[k], curved)
                for j, i in samples:
                    dense = ref.dense_umbra(scene.surface, (j, i), dirs[k], scene.inv_two_r_prime, curved)
                    # (sampling can only fall short of the supremum, by its step)
                    assert -1e-9 * (1 + abs(dense)) <= want[j, i] - dense <= 1e-3 * (1 + abs(dense)), (shape, k, curved, j, i, want[j, i], dense)


# ---- inputs with known answers -----------------------------------------------------------------------------------------------
def _exit_parameter(surface, dx, dz):
    """The parameter at which the line from every sample along (dx, dz) leaves the footprint (0: no cell beside the sample)."""
    X, Z = surface.X, surface.Z
    with np.errstate(all="ignore"):
        tx = ((X[-1] - X) / dx if dx > 0 else (X[0] - X) / dx) if dx != 0 else np.where(np.arange(len(X)) < len(X) - 1, np.inf, 0.0)
        tz = ((Z[-1] - Z) / dz if dz > 0 else (Z[0] - Z) / dz) if dz != 0 else np.where(np.arange(len(Z)) < len(Z) - 1, np.inf, 0.0)
    return np.minimum(tx[None, :], tz[:, None])


def test_planar_dem_tilted_toward_and_away(harness):
    """y = a x + b z: along (dx, dy, dz) the functional is (a dx + b dz - dy) t.  Where the plane rises faster than the ray it is
    largest at the footprint's exit; where it rises slower, or falls, the ground is lit."""
    a, b = 0.25, -0.5
    rows, cols = 17, 21
    x = (np.arange(cols, dtype=np.float64) - 0.5 * (cols - 1))[None, :]
    z = (np.arange(rows, dtype=np.float64) - 0.5 * (rows - 1))[:, None]
    dem = (a * x + b * z).astype(f32)
    scene = HostScene(harness, dem, _planar(dem, 1.0))
    try:
        dirs = np.array([[1.0, 0.1, -1.0, 0.0],    # up the plane: it rises 0.75 a unit, the ray 0.1
                         [1.0, 0.75, -1.0, 0.0],   # grazing: the slope itself
                         [1.0, 0.9, -1.0, 0.0],    # up the plane but steeper than it
                         [-1.0, 0.05, 1.0, 0.0],   # down the plane
                         [-1.0, -0.5, 1.0, 0.0],   # down the plane, descending more slowly than it falls: lit
                         [-1.0, -0.9, 1.0, 0.0],   # ... faster than it falls: the ray dives into the ground
                         [2.0, 0.3, 1.0, 0.0]], f32)  # across: the plane is level along (2, 1)
        got = scene.run(dirs, False)["depth"]
        h = scene.surface.h64
        for k, d in enumerate(dirs):
            rate = a * float(d[0]) + b * float(d[2]) - float(d[1])
            want = np.maximum(rate, 0.0) * _exit_parameter(scene.surface, float(d[0]), float(d[2]))
            compare(got[k], want, np.ones((rows, cols), bool) & (_exit_parameter(scene.surface, float(d[0]), float(d[2])) > 0), h, scene.relief)
        assert got[0].max() > 5.0 and got[5].max() > 1.0 and got[2].max() <= TOL * (1 + 2 * scene.relief)
        assert got[3].max() <= TOL * (1 + 2 * scene.relief) and got[4].max() <= TOL * (1 + 2 * scene.relief)
    finally:
        scene.close()


def test_ridge_case(harness):
    """The raster tests' ridge: 33x33, column 16 at 600 m, 3 400 m cells.  The tent has no twist, so toward +x with a rise dy a
    sample west of the ridge is lit from the height ridge - dy t - h, t its distance to the ridge; the ridge and what lies east
    of it are lit on the ground -- as is the last row, which has no cell beside it along +x.  Curved: against the reference."""
    dem = np.zeros((33, 33), f32)
    dem[:, 16] = 600.0
    scene = HostScene(harness, dem, _planar(dem, 3400.0), cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        assert scene.curvature_enabled
        X = scene.surface.X
        h = scene.surface.h64
        for dy in (0.02, 0.05):
            d = np.array([1.0, dy, 0.0, 0.0], f32)
            want = np.broadcast_to(np.where(np.arange(33) < 16, np.maximum(600.0 - float(d[1]) * (X[16] - X), 0.0), 0.0), (33, 33)).copy()
            want[32] = 0.0
            got = scene.run(d, False)["depth"][0]
            along = np.ones((33, 33), bool)
            along[32] = False
            along[:, 32] = False
            compare(got, want, along, h, scene.relief)
            assert got[5, 15] > 400.0 and (got[:, 16:] == 0).all()
            flat_ref, along = scene.reference(d, False)
            compare(got, flat_ref, along, h, scene.relief)
            curved_ref, along = scene.reference(d, True)
            curved = scene.run(d, True)["depth"][0]
            compare(curved, curved_ref, along, h, scene.relief)
            assert (curved <= got + TOL * (1 + 600 + 600)).all() and (curved < got - 1.0).any(), "the earth falls away under the ray: less shadow"
    finally:
        scene.close()


def test_the_earths_bulge_over_a_flat_dem(harness):
    """A flat DEM with curvature on and a ray that dips by a = -dy a unit: the functional is a t - k t^2, largest at
    t* = a / (2 k) where it is a^2 / (4 k) -- with k = |d_h|^2 / (2 R') the height h = s^2 / (2 R') from which the dip angle a / |d_h|
    just grazes the earth's bulge at the distance s = R' a / |d_h| -- or at the footprint's exit if that comes first.  A rising ray
    over a flat DEM is lit on the ground, and so is the dipping one under the flat policy only at the sample where it has
    nowhere to go."""
    c, a = 3.5, 0.003
    dem = np.full((17, 21), c, f32)
    scene = HostScene(harness, dem, _planar(dem, 3400.0), cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        assert scene.curvature_enabled
        d = np.array([0.6, -a, 0.8, 0.0], f32)
        k = (float(d[0]) ** 2 + float(d[2]) ** 2) * float(scene.inv_two_r_prime)
        dip = -float(d[1])
        t_exit = _exit_parameter(scene.surface, float(d[0]), float(d[2]))
        t = np.minimum(t_exit, dip / (2.0 * k))
        want = dip * t - k * t * t
        assert (t < t_exit).any() and (t == t_exit).any() and want.max() > 30.0, "samples whose ray grazes inside the footprint, and not"
        got = scene.run(d, True)["depth"][0]
        compare(got, want, t_exit > 0, scene.surface.h64, scene.relief)
        compare(scene.run(d, False)["depth"][0], dip * t_exit, t_exit > 0, scene.surface.h64, scene.relief)
        up = np.array([0.6, a, 0.8, 0.0], f32)
        for curved in (False, True):
            assert (scene.run(up, curved)["depth"][0].view(np.uint32) == 0).all(), "a rising ray over a flat DEM: lit on the ground"
    finally:
        scene.close()


# ---- regions, footprints, the cap, bad directions, deepest, the session's sun ---------------------------------------------------
@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65), (62, 0, 1, 65), (20, 20, 1, 1)])
def test_regions(shaped, region):
    scene = shaped[(63, 65)]
    dirs = directions(scene)
    whole = scene.run(dirs, True)
    r0, c0, r, c = region
    for block in (0, 1):
        got = scene.run(dirs, True, region=region, block=block)
        assert np.array_equal(got["depth"].view(np.uint32), whole["depth"][:, r0:r0 + r, c0:c0 + c].view(np.uint32)), "a window of the whole raster"
        assert np.array_equal(got["deepest"].view(np.uint32), whole["deepest"][r0:r0 + r, c0:c0 + c].view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_both_wave_footprints_give_the_same_bits(shaped, shape):
    scene = shaped[shape]
    dirs = directions(scene)
    row, block = scene.run(dirs, True, block=0), scene.run(dirs, True, block=1)
    assert np.array_equal(row["depth"].view(np.uint32), block["depth"].view(np.uint32))
    assert np.array_equal(row["deepest"].view(np.uint32), block["deepest"].view(np.uint32))
    assert not (block["depth"] == 77.0).any() and not (block["deepest"] == 77.0).any(), "every sample is written"


def deepest_f32(planes):
    """`deepest` as the contract states it: from +0, fmax over the planes in order, NaN ignored."""
    return np.fmax.reduce(np.concatenate([np.zeros((1, *planes.shape[1:]), f32), planes]))


def test_step_cap(shaped):
    """An injected tiny cap (the harness alone can): a lane whose walk is not over after `cap` steps writes qNaN for that
    direction and goes on to the next; `deepest` ignores it.  The real cap is never reached."""
    scene = shaped[(63, 65)]
    dirs = directions(scene)[:WALKED]
    full = scene.run(dirs)
    assert not np.isnan(full["depth"]).any() and not np.isnan(full["deepest"]).any()
    assert scene.step_cap == 4 * (64 + 62) + 8 * 7
    capped = scene.run(dirs, cap=3)
    nan = np.isnan(capped["depth"])
    assert nan.any() and not nan.all()
    assert (capped["depth"].view(np.uint32)[nan] == 0x7FC00000).all(), "the quiet NaN"
    assert np.array_equal(capped["depth"][~nan].view(np.uint32), full["depth"][~nan].view(np.uint32)), "a walk that ends within the cap is untouched"
    assert all(nan[k].any() and (~nan[k]).any() for k in range(WALKED)), "per direction: a lane goes on after a capped one"
    assert np.array_equal(capped["deepest"].view(np.uint32), deepest_f32(capped["depth"]).view(np.uint32))


def test_bad_directions_answer_nan(shaped):
    """The device form's path: the host never sees the directions, the lanes answer a non-finite or zero one, or one with
    w != 0, with NaN."""
    scene = shaped[(33, 33)]
    good = directions(scene)[1]
    bads = []
    for slot in range(4):
        for value in (np.nan, np.inf, -np.inf):
            bad = good.copy()
            bad[slot] = value
            bads.append(bad)
    bads += [np.zeros(4, f32), np.array([good[0], good[1], good[2], 1.0], f32), np.array([0.0, 1.0, 0.0, -2.0], f32)]
    for bad in bads:
        got = scene.run(np.stack([good, bad, good]))
        assert np.isnan(got["depth"][1]).all() and not np.isnan(got["depth"][[0, 2]]).any(), bad
        assert (got["depth"][1].view(np.uint32) == 0x7FC00000).all()
        assert np.array_equal(got["depth"][0].view(np.uint32), got["depth"][2].view(np.uint32))
        assert np.array_equal(got["deepest"].view(np.uint32), got["depth"][0].view(np.uint32)), "a NaN plane is ignored"
    alone = scene.run(np.array([[np.nan, 1.0, 2.0, 0.0]], f32))
    assert np.isnan(alone["depth"]).all() and (alone["deepest"].view(np.uint32) == 0).all(), "nothing but NaN planes: +0"
    minus_zero = scene.run(np.array([[good[0], good[1], good[2], -0.0]], f32))
    assert np.array_equal(minus_zero["depth"][0].view(np.uint32), scene.run(good)["depth"][0].view(np.uint32)), "w = -0 is 0"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_deepest_is_the_maximum_over_the_planes_bit_for_bit(shaped, shape):
    scene = shaped[shape]
    dirs = directions(scene)
    for curved in (False, True):
        for sub in (dirs, dirs[:WALKED]):
            both = scene.run(sub, curved)
            want = deepest_f32(both["depth"])
            assert np.array_equal(want.view(np.uint32), np.fmax.reduce(both["depth"]).view(np.uint32)), "every plane is >= +0: np.fmax.reduce of the planes"
            assert np.array_equal(both["deepest"].view(np.uint32), want.view(np.uint32))
            alone = scene.run(sub, curved, planes=False)
            assert alone["depth"] is None and np.array_equal(alone["deepest"].view(np.uint32), want.view(np.uint32)), "with depth null as well"
            planes_only = scene.run(sub, curved, deepest=False)
            assert np.array_equal(planes_only["depth"].view(np.uint32), both["depth"].view(np.uint32))
        assert np.isposinf(scene.run(dirs, curved)["deepest"]).all(), "straight down is among them"


def test_session_sun_is_the_armed_direction(shaped):
    scene = shaped[(64, 64)]
    assert np.isfinite(scene.sun).all() and scene.sun[1] > 0
    for curved in (False, True):
        sun = scene.run(None, curved)
        given = scene.run(np.array([[*scene.sun, 0.0]], f32), curved)
        assert np.array_equal(sun["depth"].view(np.uint32), given["depth"].view(np.uint32))
        assert np.array_equal(sun["deepest"].view(np.uint32), given["deepest"].view(np.uint32))
        assert (sun["depth"] == 0).any() and (sun["depth"] > 0).any()
        want, along = scene.reference(np.array([*scene.sun, 0.0], f32), curved)
        compare(sun["depth"][0], want, along, scene.surface.h64, scene.relief)


# ---- a second opinion on lit / shadowed: the horizon raster's host body ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 33), (63, 65)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_cross_check_with_the_horizon_walk(shaped, shape):
    """H, the horizon at lift 0 along (dx, dz), is the supremum of (y - k t^2 - h) / t, and the functional here is t times that
    minus dy: the ground is lit exactly when H <= dy.  Away from a band of rounding around H == dy -- BAND (1 + |H| + |dy|): both
    are slopes, evaluated in f32 from heights a few ulp of which the band dwarfs -- the two walks must agree; H == -inf (no terrain
    along the azimuth) is exactly +0."""
    scene = shaped[shape]
    dirs = directions(scene)[:WALKED]
    for curved in (False, True):
        L = scene.run(dirs, curved)["depth"]
        H = scene.horizon(dirs[:, [0, 2]], curved, 0.0)
        for k in range(WALKED):
            dy = float(dirs[k, 1])
            with np.errstate(invalid="ignore"):
                band = BAND * (1.0 + np.where(np.isfinite(H[k]), np.abs(H[k]), 0.0) + abs(dy))
            lit, dark = H[k] < dy - band, H[k] > dy + band
            assert (L[k][lit].view(np.uint32) == 0).all(), (NAMES[k], curved)
            assert (L[k][dark] > 0).all(), (NAMES[k], curved)
            assert (L[k][np.isneginf(H[k])].view(np.uint32) == 0).all()
            assert (lit | dark).mean() > 0.9, "the band leaves most samples in"
            assert lit.any() and (dark.any() or (k == 2 and shape == (33, 33)))  # (nothing in shadow there at elevation 30)


# ---- the bracket the GPU suite checks against visibility(), on the reference --------------------------------------------------
def band_of(lstar, h, relief):
    return BAND * (1.0 + np.where(np.isfinite(lstar), lstar, 0.0) + np.abs(h) + relief)


def left_out(lstar, rung, h, relief):
    return np.isfinite(lstar) & (np.abs(rung - lstar) <= band_of(lstar, h, relief))


def test_bracket_leaves_out_at_most_four_percent(shaped):
    """tests/test_gpu_umbra.py compares `rung > L*` with visibility(d, lift=rung) wherever |rung - L*| > 2e-3 (1 + L* + |h| +
    relief): the share of samples left out, on the float64 reference, per rung and direction."""
    assert MEASURED > 0.0 and 10.0 * TOL < BAND, f"10 x the test bound {TOL:.3g} must stay below the band {BAND:.3g}"
    lit_all = []
    for shape in ((33, 33), (63, 65)):
        scene = shaped[shape]
        dirs = directions(scene)
        for k in range(5):
            for curved in (False, True):
                lstar, _ = scene.reference(dirs[k], curved)
                h = scene.surface.h64
                shares = [float(left_out(lstar, r, h, scene.relief).mean()) for r in RUNGS]
                lit = [float((r > lstar).mean()) for r in RUNGS]
                print(f"{shape[1]}x{shape[0]} {NAMES[k]} {'curved' if curved else 'flat'}: left out " + " / ".join(f"{100 * v:.2f} %" for v in shares) +
                      "; lit " + " / ".join(f"{v:.3f}" for v in lit))
                assert max(shares) <= 0.04
                assert all(x <= y for x, y in zip(lit, lit[1:]))
                lit_all += lit
    assert min(lit_all) < 0.6 and max(lit_all) > 0.9, "the rungs cut through the distribution"


# ---- the sanitizer run: a stand-alone program, never code loaded into this process ---------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(HARNESS, "umbra")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "NaN without an injected cap or a bad direction: 0" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- the interface -------------------------------------------------------------------------------------------------------------
MEMBERS = ["struct_size", "flags", "row0", "col0", "rows", "cols", "direction_count", "reserved", "directions", "depth", "deepest"]


def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header, "the umbra raster is additive: no ABI version bump"
    body = re.search(r"typedef struct f3d_session_umbra_desc \{(.*?)\} f3d_session_umbra_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [name for name, _ in _native.UmbraDesc._fields_] == MEMBERS
    assert C.sizeof(_native.UmbraDesc) == 56 == harness.umbra_desc_size()
    assert _native.UmbraDesc.direction_count.offset == 24 and _native.UmbraDesc.reserved.offset == 28
    assert _native.UmbraDesc.directions.offset == 32 and _native.UmbraDesc.depth.offset == 40 and _native.UmbraDesc.deepest.offset == 48
    assert re.search(r"int f3d_session_umbra\(f3d_session \*session, const f3d_session_umbra_desc \*desc, char \*err, size_t errlen\);", header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_umbra"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for name, value in (("CURVED", 2), ("DEVICE_POINTERS", 4), ("NO_WAIT", 8), ("SESSION_SUN", 16)):
        assert re.search(rf"#define F3D_UMBRA_{name} {value}u", header) and getattr(_native, f"UMBRA_{name}") == value
    assert _native.UMBRA_CURVED == _native.RASTER_CURVED and _native.UMBRA_DEVICE_POINTERS == _native.RASTER_DEVICE_POINTERS
    assert _native.UMBRA_NO_WAIT == _native.RASTER_NO_WAIT and _native.UMBRA_SESSION_SUN == _native.RASTER_SESSION_SUN, "the raster's flag values"
    assert "csrc/f3d_umbra.h" in header, "the ABI header refers to the contract"


def test_integration_guide_has_the_struct_and_the_extern():
    text = (ROOT / "INTEGRATION.md").read_text()
    body = re.search(r"pub struct F3dSessionUmbraDesc \{(.*?)\n\}", text, re.S).group(1)
    names = re.findall(r"pub (\w+):", body)
    assert names == MEMBERS
    types = dict(re.findall(r"pub (\w+): ([^,]+),", body))
    assert types["directions"].strip() == "*const f32" and types["depth"].strip() == "*mut f32" and types["deepest"].strip() == "*mut f32"
    assert all(types[n].strip() == "u32" for n in MEMBERS[:8])
    assert re.search(r"pub fn f3d_session_umbra\(session: \*mut F3dSession, desc: \*const F3dSessionUmbraDesc, err: \*mut c_char, errlen: usize\) -> c_int;", text)


def test_wrapper_has_the_umbra_methods():
    import inspect

    from forge3d_amd.session import TerrainSession

    p = inspect.signature(TerrainSession.umbra).parameters
    assert list(p)[:2] == ["self", "directions"] and p["directions"].default is None
    assert p["curved"].default is True and p["region"].default is None and p["planes"].default is True
    assert p["deepest"].default is False and p["wait"].default is True
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("curved", "region", "planes", "deepest", "wait"))
    v = inspect.signature(TerrainSession.lit_height).parameters
    assert list(v)[:2] == ["self", "direction"] and v["direction"].default is None
    assert v["curved"].default is True and v["region"].default is None
    for method in (TerrainSession.umbra, TerrainSession.lit_height):
        assert "shadow_mask(d) == (lit_height(d) < SURFACE_BIAS)" in " ".join(method.__doc__.split())
