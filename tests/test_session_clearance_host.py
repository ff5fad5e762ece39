"""Clearance rasters on a live terrain session (f3d_session_clearance), the parts that need no GPU.

The lane body of the clearance kernel (csrc/f3d_clearance.h clearance_lane, what k_clearance calls per lane) compiled for the
host (tests/clearance_host) and run over the kernel's waves and lanes (csrc/f3d_walk.h region_sample), against
tests/clearance_reference.py -- an independent float64 statement of the contract's first form that cuts the sight line at
every lattice line and knows nothing of the pyramid or the walk.

* DEMs 5x3, 33x33, 64x64 and 65x63 (test_session_raster_host.SHAPES, its spacing and exaggeration), curved and flat; seven
  observers (`observers` below): the three of viewshed_targets (high over the footprint; with a distance limit; exactly on a
  lifted sample), one outside the footprint, one whose x is exactly a lattice column (a column of dx == 0 walks), one on the
  DEM's last lattice line, one well under the surface (every sample +inf);
* +inf exactly where the reference has it, no NaN, exactly 0 where the reference has no terrain between, elsewhere
  |L - L64| <= TOL (1 + |L64| + |Y| + |h|) -- the rounding floor is an ulp of the heights, not of L.  TOL is 8 x the largest
  such ratio MEASURED over exactly these inputs: see MEASURED below and DESIGN.md;
* inputs with known answers (a planar DEM, the raster tests' ridge, the earth's bulge over a flat DEM), regions, both wave
  footprints, the step cap (injected here only), NaN observers, `lowest`, the reference itself against dense sampling, and
  the share of samples the GPU suite's bracket test has to leave out, on the reference;
* a stand-alone driver (its own main) of the same lane body built with -fsanitize=address,undefined and run once;
* the header, the ctypes table and the descriptor's layout; the wrapper's methods.
The refusals of f3d_session_clearance need a session, i.e. a device: tests/test_gpu_clearance.py.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import clearance_reference as ref
import scenes
from emul import emul
from test_session_raster_host import SHAPES, _kw, _planar, contract_origins, shaped_dem, viewshed_targets
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "clearance_host" / "clearance_harness.cpp"
SIZE = (96, 64)
CURVED = 2
f32 = np.float32

# The largest |L - L64| / (1 + |L64| + |Y| + |h|) of the host body against the float64 reference over the seven observers x
# curved / flat x SHAPES, measured (test_host_body_against_the_reference prints each case's: 64x64, flat, the observer on a
# last lattice line); the bound is 8 x it.  10 x TOL = 2.4e-4 stays below the 2e-3 band the GPU suite's bracket leaves out.
MEASURED = 2.98e-6
TOL = 8.0 * MEASURED
RUNGS = (0.25, 1.0, 3.0, 8.0)  # the bracket test's lifts (tests/test_gpu_clearance.py)
BAND = 2e-3


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "clearance_host")
    lib.clearance_scene_create.restype = C.c_void_p
    lib.clearance_scene_create.argtypes = [C.c_void_p, C.c_void_p]
    lib.clearance_scene_destroy.argtypes = [C.c_void_p]
    lib.clearance_run.restype = C.c_int
    lib.clearance_run.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 4 + [C.c_uint32] * 2
    lib.clearance_step_cap_of.restype = C.c_uint32
    lib.clearance_step_cap_of.argtypes = [C.c_void_p]
    lib.clearance_desc_size.restype = C.c_uint32
    return lib


class HostScene:
    """A scene as the emulator sets it up, and clearance rasters over it as f3d_session_clearance's device form answers them."""

    def __init__(self, lib, dem, kw, cam=None):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        d, keep = _desc(self.dem, SIZE, cam or scenes.CAM, kw)
        info = np.zeros(6, f32)
        self.handle = lib.clearance_scene_create(C.addressof(d), info.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin, self.spacing = (f32(info[0]), f32(info[1])), (f32(info[2]), f32(info[3]))
        self.inv_two_r_prime, self.curvature_enabled = f32(info[4]), bool(info[5])
        self.surface = ref.Surface(self.dem, kw["exaggeration"], self.origin, self.spacing)
        self.step_cap = int(lib.clearance_step_cap_of(self.handle))
        self._reference = {}

    def close(self):
        self.lib.clearance_scene_destroy(self.handle)

    def region(self, region):
        return (0, 0, *self.dem.shape) if region is None else tuple(int(v) for v in region)

    def run(self, observers, curved=False, region=None, planes=True, lowest=True, cap=0, block=0):
        row0, col0, rows, cols = self.region(region)
        ob = np.ascontiguousarray(observers, f32).reshape(-1, 4)
        k, n = len(ob), rows * cols
        h = np.full((k, n), 77.0, f32) if planes else None
        low = np.full(n, 77.0, f32) if lowest else None
        g = np.full((n, 3), 77.0, f32)
        assert self.lib.clearance_run(self.handle, CURVED if curved else 0, row0, col0, rows, cols, k, ob.ctypes.data,
                                      h.ctypes.data if planes else None, low.ctypes.data if lowest else None, g.ctypes.data, cap, block) == 0
        return {"height": h.reshape(k, rows, cols) if planes else None, "lowest": low.reshape(rows, cols) if lowest else None,
                "samples": g.reshape(rows, cols, 3)}

    def reference(self, observer, curved):
        """(L64, between) of one observer over the whole DEM: computed once, shared, never written to."""
        key = (np.asarray(observer, f32).tobytes(), bool(curved))
        if key not in self._reference:
            got = ref.clearance_reference(self.surface, self.region(None), observer, self.inv_two_r_prime, curved and self.curvature_enabled,
                                          return_between=True)
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


NAMES = ("over", "limited", "on a sample", "outside", "on a lattice column", "on the last lattice line", "under the surface")


def observers(scene):
    """The seven observers of the module's docstring, (7, 4) float32, in the order of NAMES."""
    ox = float(scene.origin[0])
    rows, cols = scene.dem.shape
    three, _ = viewshed_targets(scene)
    X, Z = scene.surface.X, scene.surface.Z
    low = float(scene.surface.h.min())
    more = np.array([[1.4 * ox, 9.0, -0.3 * ox, 0.0],
                     [X[cols // 2], 14.0, 0.37 * float(scene.origin[1]), 0.0],
                     [0.11 * ox, 15.0, Z[rows - 1], 0.0],
                     [0.13 * ox, low - 5.0, 0.17 * float(scene.origin[1]), 0.0]], f32)
    assert more[1, 0] == f32(X[cols // 2]) and more[2, 2] == f32(Z[rows - 1])
    return np.concatenate([three, more]).astype(f32)


def compare(got, want, between, Y, h, tol=TOL):
    """+inf where the reference has it, no NaN, exactly 0 without terrain between, elsewhere the bound; returns the largest ratio."""
    assert not np.isnan(got).any(), "no NaN"
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), "+inf exactly where the reference has +inf"
    assert not np.isneginf(got).any() and (got >= 0).all()
    none = ~between & np.isfinite(want)
    assert (got[none] == 0.0).all() and (want[none] == 0.0).all(), "exactly 0 where no terrain lies between"
    fin = np.isfinite(want)
    ratio = np.abs(got[fin].astype(np.float64) - want[fin]) / (1.0 + np.abs(want[fin]) + abs(float(Y)) + np.abs(h[fin]))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= tol, f"|L - L64| / (1 + |L64| + |Y| + |h|) reaches {worst:.3g}, the bound is {tol:.3g}"
    return worst


# ---- the host body against the float64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_host_body_against_the_reference(shaped, shape, curved):
    scene = shaped[shape]
    assert scene.curvature_enabled and scene.inv_two_r_prime > 0.0
    obs = observers(scene)
    got = scene.run(obs, curved)
    want_g = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, scene.region(None), 0.0)
    assert np.array_equal(got["samples"].view(np.uint32), want_g.view(np.uint32)), "the rasters' lattice points, lift 0"
    h = scene.surface.h64
    for k, name in enumerate(NAMES):
        want, between = scene.reference(obs[k], curved)
        worst = compare(got["height"][k], want, between, obs[k, 1], h)
        print(f"{shape[1]}x{shape[0]} {'curved' if curved else 'flat'} {name}: largest ratio {worst:.3g} (bound {TOL:.3g}), "
              f"{int(np.isposinf(want).sum())} +inf, {int((want == 0).sum())} zero of {want.size}")
    assert np.isposinf(got["height"][6]).all(), "an observer well under the surface sees nothing at any height"
    rows, cols = scene.dem.shape
    if rows * cols > 64:
        assert np.isposinf(got["height"][1]).any() and np.isfinite(got["height"][1]).any(), "the distance limit cuts part of the raster"
        first = got["height"][0]
        assert (first == 0).any() and (first > 0).any()
    on = (rows // 2, cols // 3)
    assert got["height"][2][on] == 0.0, "the sample straight under the observer"


def test_curvature_raises_the_clearance(shaped):
    scene = shaped[(63, 65)]
    ob = observers(scene)[:1]
    flat, curved = scene.run(ob, False)["height"], scene.run(ob, True)["height"]
    assert not np.array_equal(flat, curved)
    assert (curved >= flat - TOL * (1 + np.abs(flat) + 16 + np.abs(scene.surface.h64))).all(), "the bulge hides, it never reveals"


def test_reference_against_dense_sampling(shaped):
    """The reference's closed form per segment against brute force: 4000 parameters a cell along the line."""
    for shape, samples in (((3, 5), [(0, 0), (1, 2), (2, 4), (1, 0)]), ((33, 33), [(16, 16), (3, 30), (32, 0), (0, 32), (20, 7)])):
        scene = shaped[shape]
        obs = observers(scene)
        for k in (0, 2, 3, 4, 5):
            for curved in (False, True):
                want, _ = scene.reference(obs[k], curved)
                for j, i in samples:
                    if not np.isfinite(want[j, i]) or (obs[k, 0] == f32(scene.surface.X[i]) and obs[k, 2] == f32(scene.surface.Z[j])):
                        continue
                    dense = ref.dense_clearance(scene.surface, (j, i), obs[k], scene.inv_two_r_prime, curved)
                    # (sampling can only fall short of the supremum, by its step)
                    assert -1e-5 * (1 + abs(dense)) <= want[j, i] - dense <= 1e-3 * (1 + abs(dense)), (shape, k, curved, j, i, want[j, i], dense)


# ---- inputs with known answers -----------------------------------------------------------------------------------------------
def test_planar_dem_seen_from_above(harness):
    """y = a x + b z seen from above the plane: the ground shows everywhere, every value within the bound of 0."""
    a, b = 0.25, -0.5
    rows, cols = 17, 21
    x = (np.arange(cols, dtype=np.float64) - 0.5 * (cols - 1))[None, :]
    z = (np.arange(rows, dtype=np.float64) - 0.5 * (rows - 1))[:, None]
    dem = (a * x + b * z).astype(f32)
    scene = HostScene(harness, dem, _planar(dem, 1.0))
    try:
        obs = np.array([[1.3, 9.0, -2.2, 0.0], [-14.0, 4.0, 3.0, 0.0], [2.0, a * 2.0 + b * 1.0 + 0.5, 1.0, 0.0], [0.0, 6.0, 0.0, 5.0]], f32)
        for curved in (False, True):
            got = scene.run(obs, curved)["height"]
            for k in range(len(obs)):
                fin = np.isfinite(got[k])
                assert fin.all() or k == 3
                bound = TOL * (1.0 + abs(float(obs[k, 1])) + np.abs(scene.surface.h64))
                assert (got[k][fin] <= bound[fin]).all() and (got[k][fin] >= 0).all(), (k, float(got[k][fin].max()))
    finally:
        scene.close()


def test_ridge_case(harness):
    """The raster tests' ridge: 33x33, column 16 at 600 m, 3 400 m cells, the observer 100 m up at column 3.2 of row 16.  The
    tent has no twist, so by similar triangles a sample behind the ridge needs Y + (600 - Y)(x - x_o) / (x_ridge - x_o); in
    front of it, and on it, the ground shows.  Curved: against the reference."""
    dem = np.zeros((33, 33), f32)
    dem[:, 16] = 600.0
    scene = HostScene(harness, dem, _planar(dem, 3400.0), cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        assert scene.curvature_enabled
        ob = np.array([float(scene.origin[0]) + 3.2 * 3400.0, 100.0, float(scene.origin[1]) + 16 * 3400.0, 0.0], f32)
        X = scene.surface.X
        xo, Y = float(ob[0]), float(ob[1])
        want = np.broadcast_to(np.where(np.arange(33) > 16, Y + (600.0 - Y) * (X - xo) / (X[16] - xo), 0.0), (33, 33))
        got = scene.run(ob, False)["height"][0]
        h = scene.surface.h64
        compare(got, want, np.ones((33, 33), bool), Y, h)
        assert (got[:, :17] <= TOL * (1 + Y + 600)).all() and got[16, 24] > 600.0
        flat_ref, between = scene.reference(ob, False)
        compare(got, flat_ref, between, Y, h)
        curved_ref, between = scene.reference(ob, True)
        curved = scene.run(ob, True)["height"][0]
        compare(curved, curved_ref, between, Y, h)
        assert (curved[:, :14] > 0).any(), "the curvature hides far ground in front of the ridge too"
    finally:
        scene.close()


def test_the_earths_bulge_over_a_flat_dem(harness):
    """A flat DEM at height c with curvature on, the observer a = Y - c above it at horizontal distance D: the contract's
    first form is sup_t k t - a t / (1 - t) with k = D^2 inv_two_r_prime, stationary at 1 - t = sqrt(a / k), so
        L* = max(0, sqrt(k) - sqrt(a))^2 = max(0, D - sqrt(2 R' a))^2 / (2 R'):
    the classical height hidden by the earth's bulge beyond the observer's horizon distance sqrt(2 R' a)."""
    c, a = 3.5, 2.0
    dem = np.full((17, 21), c, f32)
    scene = HostScene(harness, dem, _planar(dem, 3400.0), cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        assert scene.curvature_enabled
        ob = np.array([0.31 * float(scene.origin[0]), c + a, 0.23 * float(scene.origin[1]), 0.0], f32)
        region = scene.region(None)
        k = ref.sample_geometry(scene.surface, region, ob, scene.inv_two_r_prime, True)[-1].reshape(17, 21)
        want = np.maximum(np.sqrt(k) - np.sqrt(a), 0.0) ** 2
        assert (want > 1.0).any() and (want == 0.0).any(), "samples beyond the horizon distance and within it"
        got = scene.run(ob, True)["height"][0]
        compare(got, want, np.ones((17, 21), bool), ob[1], scene.surface.h64)
        assert (scene.run(ob, False)["height"][0] == 0.0).all(), "flat policy: a flat DEM shows everywhere"
    finally:
        scene.close()


# ---- regions, footprints, the cap, NaN, lowest ----------------------------------------------------------------------------------
@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65), (20, 20, 1, 1)])
def test_regions(shaped, region):
    scene = shaped[(63, 65)]
    obs = observers(scene)
    whole = scene.run(obs, True)
    r0, c0, r, c = region
    for block in (0, 1):
        got = scene.run(obs, True, region=region, block=block)
        assert np.array_equal(got["height"].view(np.uint32), whole["height"][:, r0:r0 + r, c0:c0 + c].view(np.uint32)), "a window of the whole raster"
        assert np.array_equal(got["lowest"].view(np.uint32), whole["lowest"][r0:r0 + r, c0:c0 + c].view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_both_wave_footprints_give_the_same_bits(shaped, shape):
    scene = shaped[shape]
    obs = observers(scene)
    row, block = scene.run(obs, True, block=0), scene.run(obs, True, block=1)
    assert np.array_equal(row["height"].view(np.uint32), block["height"].view(np.uint32))
    assert np.array_equal(row["lowest"].view(np.uint32), block["lowest"].view(np.uint32))
    assert not (block["height"] == 77.0).any() and not (block["lowest"] == 77.0).any(), "every sample is written"


def test_step_cap(shaped):
    """An injected tiny cap (the harness alone can): a lane whose walk is not over after `cap` steps writes qNaN for that
    observer and goes on to the next; `lowest` ignores it.  The real cap is never reached."""
    scene = shaped[(63, 65)]
    obs = observers(scene)
    full = scene.run(obs)
    assert not np.isnan(full["height"]).any() and not np.isnan(full["lowest"]).any()
    assert scene.step_cap == 4 * (64 + 62) + 8 * 7
    capped = scene.run(obs, cap=3)
    nan = np.isnan(capped["height"])
    assert nan.any() and not nan.all()
    assert (capped["height"].view(np.uint32)[nan] == 0x7FC00000).all(), "the quiet NaN"
    assert np.array_equal(capped["height"][~nan].view(np.uint32), full["height"][~nan].view(np.uint32)), "a walk that ends within the cap is untouched"
    assert nan[0].any() and (~nan[3]).any(), "per observer: a lane goes on after a capped one"
    assert np.array_equal(capped["lowest"].view(np.uint32), lowest_f32(capped["height"]).view(np.uint32))


def lowest_f32(planes):
    """`lowest` as the contract states it: from +inf, fmin over the planes in order, NaN ignored."""
    out = np.full(planes.shape[1:], np.inf, f32)
    for plane in planes:
        out = np.fmin(out, plane)
    return out


def test_nan_observers_answer_nan(shaped):
    """The device form's path: the host never sees the observers, the lanes answer a non-finite one with NaN."""
    scene = shaped[(33, 33)]
    good = observers(scene)[0]
    for slot in range(4):
        for value in (np.nan, np.inf, -np.inf):
            bad = good.copy()
            bad[slot] = value
            got = scene.run(np.stack([good, bad, good]))
            assert np.isnan(got["height"][1]).all() and not np.isnan(got["height"][[0, 2]]).any(), (slot, value)
            assert np.array_equal(got["height"][0].view(np.uint32), got["height"][2].view(np.uint32))
            assert np.array_equal(got["lowest"].view(np.uint32), got["height"][0].view(np.uint32)), "a NaN plane is ignored"
    alone = scene.run(np.array([[np.nan, 1.0, 2.0, 0.0]], f32))
    assert np.isnan(alone["height"]).all() and np.isposinf(alone["lowest"]).all(), "nothing but NaN planes: +inf"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_lowest_is_the_minimum_over_the_planes_bit_for_bit(shaped, shape):
    scene = shaped[shape]
    obs = observers(scene)
    for curved in (False, True):
        both = scene.run(obs, curved)
        want = lowest_f32(both["height"])
        assert np.array_equal(both["lowest"].view(np.uint32), want.view(np.uint32))
        alone = scene.run(obs, curved, planes=False)
        assert alone["height"] is None and np.array_equal(alone["lowest"].view(np.uint32), want.view(np.uint32)), "with height null as well"
        planes_only = scene.run(obs, curved, lowest=False)
        assert np.array_equal(planes_only["height"].view(np.uint32), both["height"].view(np.uint32))


# ---- the bracket the GPU suite checks against visibility(), on the reference --------------------------------------------------
def band_of(lstar, Y, h):
    return BAND * (1.0 + np.abs(np.where(np.isfinite(lstar), lstar, 0.0)) + abs(float(Y)) + h)


def left_out(lstar, rung, Y, h):
    return np.isfinite(lstar) & (np.abs(rung - lstar) <= band_of(lstar, Y, h))


def test_bracket_leaves_out_at_most_two_percent(shaped):
    """tests/test_gpu_clearance.py compares `L > L*` with visibility(lift=L) wherever |L - L*| > 2e-3 (1 + |L*| + |Y| + h): the
    share of samples left out, on the float64 reference, per rung and observer."""
    assert 10.0 * TOL < BAND, f"10 x the test bound {TOL:.3g} must stay below the band {BAND:.3g}"
    seen_all = []
    for shape in ((33, 33), (63, 65)):
        scene = shaped[shape]
        obs = observers(scene)
        for k in (0, 1, 2, 3):
            for curved in (False, True):
                lstar, _ = scene.reference(obs[k], curved)
                h = scene.surface.h64
                shares = [float(left_out(lstar, r, obs[k, 1], h).mean()) for r in RUNGS]
                in_range = np.isfinite(lstar) if k == 1 else np.ones(lstar.shape, bool)
                seen = [float((r > lstar)[in_range].mean()) for r in RUNGS]
                print(f"{shape[1]}x{shape[0]} {NAMES[k]} {'curved' if curved else 'flat'}: left out " + " / ".join(f"{100 * v:.2f} %" for v in shares) +
                      "; seen " + " / ".join(f"{v:.3f}" for v in seen))
                assert max(shares) <= 0.02
                assert all(x <= y for x, y in zip(seen, seen[1:]))
                seen_all += seen
    assert min(seen_all) < 0.5 and max(seen_all) > 0.9, "the rungs cut through the distribution"


# ---- the sanitizer run: a stand-alone program, never code loaded into this process ---------------------------------------------
def test_driver_runs_clean_under_address_and_undefined_sanitizers():
    run = emul.run_sanitized_driver(HARNESS, "clearance")
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert "NaN without an injected cap or a NaN observer: 0" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header, "the clearance raster is additive: no ABI version bump"
    body = re.search(r"typedef struct f3d_session_clearance_desc \{(.*?)\} f3d_session_clearance_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [name for name, _ in _native.ClearanceDesc._fields_]
    assert members == ["struct_size", "flags", "row0", "col0", "rows", "cols", "observer_count", "observers", "height", "lowest", "reserved"]
    assert C.sizeof(_native.ClearanceDesc) == 64 == harness.clearance_desc_size()
    assert _native.ClearanceDesc.observer_count.offset == 24 and _native.ClearanceDesc.observers.offset == 32
    assert _native.ClearanceDesc.height.offset == 40 and _native.ClearanceDesc.lowest.offset == 48 and _native.ClearanceDesc.reserved.offset == 56
    assert re.search(r"int f3d_session_clearance\(f3d_session \*session, const f3d_session_clearance_desc \*desc, char \*err, size_t errlen\);", header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_clearance"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for name, value in (("CURVED", 2), ("DEVICE_POINTERS", 4), ("NO_WAIT", 8)):
        assert re.search(rf"#define F3D_CLEARANCE_{name} {value}u", header) and getattr(_native, f"CLEARANCE_{name}") == value
    assert _native.CLEARANCE_CURVED == _native.RASTER_CURVED and _native.CLEARANCE_DEVICE_POINTERS == _native.RASTER_DEVICE_POINTERS
    assert _native.CLEARANCE_NO_WAIT == _native.RASTER_NO_WAIT, "the raster's flag values"


def test_wrapper_has_the_clearance_methods():
    import inspect

    from forge3d_amd.session import TerrainSession

    p = inspect.signature(TerrainSession.clearance).parameters
    assert list(p)[:2] == ["self", "observers"]
    assert p["curved"].default is False and p["region"].default is None and p["planes"].default is True
    assert p["lowest"].default is False and p["wait"].default is True
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("curved", "region", "planes", "lowest", "wait"))
    v = inspect.signature(TerrainSession.visible_height).parameters
    assert list(v)[:2] == ["self", "observer"]
    assert v["observer_height"].default == 1.7 and v["max_distance"].default is None and v["curved"].default is False and v["region"].default is None
    for method in (TerrainSession.clearance, TerrainSession.visible_height):
        assert "viewshed(obs, target_height=th) == (visible_height(obs) < th + SURFACE_BIAS)" in " ".join(method.__doc__.split())
