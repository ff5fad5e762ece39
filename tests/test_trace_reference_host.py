"""The ray march against a float64 geometric reference (tests/trace_reference.py), the parts that need no GPU.

a. the reference against its own dense brute force (about 60 rays over the golden DEM, a terrace DEM with flat cells and a
   2x2 DEM; curved, vertical, starting outside the footprint, cut by tmax inside a cell);
b. the oracle (oracle/f3d_oracle.c) against the reference -- this pins the oracle to geometry, and it is where the two
   tolerances of trace_reference.py are measured;
c. the kernel's lane bodies on the host against the reference, same sets, same gates: tests/query_host (closest hit and
   occlusion), the emulator's march (any_hit 2, 3, 6, 7) and tests/raster_host (whole rasters).

The sets are generic by construction -- no azimuth is a multiple of 45 degrees, no origin or direction is lattice-aligned
except where a raster puts the start on a lattice point -- and lie outside what the reference shader answers by a policy of
its own: no ray starts on or under the surface (hybrid_terrain_traversal.wgsl:197-201; asserted: 0 per set), and rays whose
clearance is within 1e-5 of the relief are left out of the hit/miss gate (asserted: at most 0.5 % per set).  The
adversarial, lattice-aligned sets stay with the bit-for-bit tests.

Every set prints one line "trace-ref <set> <what>: rays, band share, largest height residual (in ulp(max(|o.y|, max
height))), largest normal angle, disagreements"; the disagreement count must be 0.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import scenes
import trace_reference as tr
from emul import emul
from oracle import oracle
from test_session_query_host import HARNESS as QUERY_HARNESS
from test_session_query_host import HostScene as QueryScene
from test_session_query_host import _kw
from test_session_raster_host import ALONG, CURVED, TOWARD, contract_origins, contract_rays, shaped_dem, sun_direction, viewshed_targets
from test_session_raster_host import HARNESS as RASTER_HARNESS
from test_session_raster_host import HostScene as RasterScene

f32, f64 = np.float32, np.float64
PROOF_CAM = {"origin": (0.0, 9000.0, 90000.0), "look_at": (0.0, 900.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}
# rows x cols -> spacing (None: the golden scene's span over the columns); all at exaggeration 20
SHAPES = {"2x2": ((2, 2), None), "3x5": ((3, 5), None), "63x65": ((63, 65), None), "17x130": ((17, 130), None),
          "33x33": ((33, 33), (1.5, 2.25)), "64x64": ((64, 64), None)}
RASTER_SHAPES = ("2x2", "3x5", "63x65", "17x130", "33x33")
SUNS = ((37.0, 5.0), (211.0, 15.0), (123.0, 30.0))
LIFTS = (0.5, 1e-3)
N_LIST = 1500


@functools.lru_cache(maxsize=None)
def query_lib():
    lib = emul.build_harness(QUERY_HARNESS, "query_host")
    lib.query_scene_create.restype = C.c_void_p
    lib.query_scene_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.query_scene_destroy.argtypes = [C.c_void_p]
    lib.query_run.restype = C.c_int
    lib.query_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8
    return lib


@functools.lru_cache(maxsize=None)
def raster_lib():
    lib = emul.build_harness(RASTER_HARNESS, "raster_host")
    lib.raster_scene_create.restype = C.c_void_p
    lib.raster_scene_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.raster_scene_destroy.argtypes = [C.c_void_p]
    lib.raster_run.restype = C.c_int
    lib.raster_run.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_float, C.c_uint32] + [C.c_void_p] * 5
    return lib


# ---- the scenes and the sets ------------------------------------------------------------------------------------------------
def centred_origin(dem, spacing):
    """Where a session puts the DEM: centred on the world origin, in float32 (terrain_heightfield.rs:359-360)."""
    rows, cols = dem.shape
    sx, sz = f32(spacing[0]), f32(spacing[1])
    return (f32(f32(-0.5) * (f32(cols) - f32(1.0))) * sx, f32(f32(-0.5) * (f32(rows) - f32(1.0))) * sz)


def shape_scene(name):
    """(dem, kw) of one of SHAPES: the golden DEM's relief cropped / tiled, exaggeration 20."""
    shape, spacing = SHAPES[name]
    dem = shaped_dem(shape)
    kw = _kw(dem)
    assert kw["exaggeration"] == 20.0
    if spacing is not None:
        kw["spacing"] = spacing
    return dem, kw


def reterrain_case():
    """The 64x64 golden DEM, a rougher 16x16 patch for its sample (20, 20), and the DEM that results."""
    dem = scenes.golden_dem(4)
    assert dem.shape == (64, 64)
    rng = np.random.default_rng(5)
    patch = (dem[20:36, 20:36] + rng.uniform(0.05, 0.3, (16, 16))).astype(f32)
    result = dem.copy()
    result[20:36, 20:36] = patch
    return dem, patch, result


def proof_scene():
    heights, rays = scenes.proof_rays(n_random=2000, mask=False)
    kw = dict(_kw(heights), spacing=(500.0, 500.0), exaggeration=1.0)
    origin = centred_origin(heights, kw["spacing"])
    rays = rays.copy()  # the session centres the DEM: the rays move with it, in f32
    rays[:, 0] += origin[0]
    rays[:, 2] += origin[1]
    return heights, kw, rays


def describe(dem, kw, inv_two_r_prime):
    """What the reference and the oracle need of a scene: the f32 frame, the Surface, the band's eps."""
    spacing = (f32(kw["spacing"][0]), f32(kw["spacing"][1]))
    origin = centred_origin(dem, spacing)
    surface = tr.Surface(dem, kw["exaggeration"], (float(origin[0]), float(origin[1])), (float(spacing[0]), float(spacing[1])))
    return SimpleNamespace(dem=np.ascontiguousarray(dem, f32), kw=kw, origin=origin, spacing=spacing, surface=surface,
                           inv_two_r_prime=f32(inv_two_r_prime), curvature_enabled=True, eps=tr.BAND * tr.relief(surface))


def list_rays(scene, seed, n=N_LIST):
    """n seeded generic rays over a scene, from above and from beside the footprint, aimed into it: a quarter start outside
    the footprint, a tenth point upward, a tenth have tmax drawn inside the footprint; tmin = 1e-3; directions are not
    normalised (t is in units of |d|).  Candidates that enter the footprint on or under the surface (within 1e-3 of the
    relief, decided on the f64 surface) are drawn again: the generator's rule, so that the set holds none."""
    s = scene.surface
    rng = np.random.default_rng(seed)
    x0, x1, z0, z1 = s.X[0], s.X[-1], s.Z[0], s.Z[-1]
    span = max(x1 - x0, z1 - z0)
    lo, rel = float(s.h64.min()), max(tr.relief(s), 1e-3)
    kept = []
    while sum(len(k) for k in kept) < n:
        m = 2 * n
        inside = np.stack([rng.uniform(x0, x1, m), rng.uniform(z0, z1, m)], 1)
        o = np.empty((m, 3))
        outside = rng.random(m) < 0.25
        side = rng.integers(0, 4, m)
        away = rng.uniform(0.1, 0.6, m) * span
        ox = np.where(side == 0, x0 - away, np.where(side == 1, x1 + away, inside[:, 0]))
        oz = np.where(side == 2, z0 - away, np.where(side == 3, z1 + away, inside[:, 1]))
        o[:, 0], o[:, 2] = np.where(outside, ox, inside[:, 0]), np.where(outside, oz, inside[:, 1])
        ground = s.height(np.clip(o[:, 0], x0, x1), np.clip(o[:, 2], z0, z1))
        o[:, 1] = np.where(outside, lo + rel * rng.uniform(0.3, 2.0, m), ground + rel * rng.uniform(0.02, 1.5, m))
        target = np.stack([rng.uniform(x0, x1, m), lo + rel * rng.uniform(-0.3, 1.2, m), rng.uniform(z0, z1, m)], 1)
        upward = rng.random(m) < 0.1
        target[:, 1] = np.where(upward, o[:, 1] + rel * rng.uniform(0.02, 0.5, m), target[:, 1])
        scale = rng.uniform(0.5, 2.0, m)
        d = (target - o) * scale[:, None]
        cut = rng.random(m) < 0.1
        tmax = np.where(cut, rng.uniform(0.3, 1.0, m) / scale, 1e30)
        rays = np.zeros((m, 8), f32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-3, d, tmax
        az = np.degrees(np.arctan2(rays[:, 6].astype(f64), rays[:, 4].astype(f64)))
        generic = np.abs(az / 45.0 - np.round(az / 45.0)) > 1e-3
        start = tr.terrain_reference(s, rays)["start"]
        kept.append(rays[generic & (start > 1e-3 * rel)])
    return np.concatenate(kept)[:n]


def raster_rays(scene, curved):
    """The rays of whole rasters over a scene as the contract builds them (tmin = 0): two observers (one with a distance
    limit) and three generic suns, lifts 0.5 and 1e-3.  Only the rays that march."""
    observers, _ = viewshed_targets(scene, 2)
    targets = [(TOWARD, t) for t in observers] + [(ALONG, sun_direction(az, el)) for az, el in SUNS]
    region = (0, 0, *scene.dem.shape)
    out = []
    for lift in LIFTS:
        o = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, region, lift)
        for mode, target in targets:
            rays, go = contract_rays(o, mode, target, curved, scene.inv_two_r_prime, scene.curvature_enabled)
            out.append(rays[go])
    return np.concatenate(out)


class TraceSet:
    """One set of rays over one scene with the reference's answers, flat and curved, computed once and never written."""

    def __init__(self, name, scene, rays, raster=False, rays_curved=None, which=(False, True)):
        self.name, self.scene, self.raster = name, scene, raster
        self.rays = {False: np.ascontiguousarray(rays, f32), True: np.ascontiguousarray(rays if rays_curved is None else rays_curved, f32)}
        self.ref = {}
        for curved in which:  # (a set used under one policy only pays for one)
            self.rays[curved].setflags(write=False)
            self.ref[curved] = tr.terrain_reference(scene.surface, self.rays[curved], float(scene.inv_two_r_prime), curved)
            for v in self.ref[curved].values():
                v.setflags(write=False)

    def band(self, curved):
        """Rays left out of the hit/miss gate: |clear| < eps; a lit raster sample is measured from the first lattice crossing on."""
        ref, eps = self.ref[curved], self.scene.eps
        if self.raster:
            return np.where(ref["clear"] > 0.0, ref["clear_far"] < eps, -ref["clear"] < eps)
        return np.abs(ref["clear"]) < eps

    def conditions(self, curved):
        """The stated conditions, asserted: no ray starts on or under the surface, the band holds at most 0.5 % of the set."""
        under = int((self.ref[curved]["start"] <= self.scene.eps).sum())
        assert under == 0, f"{self.name}: {under} rays start on or under the surface"
        share = float(self.band(curved).mean())
        assert share <= tr.BAND_CAP, f"{self.name}: {100 * share:.2f} % of the rays are inside the band"
        return share


def oracle_batch(scene, rays, any_hit, curved):
    return oracle.terrain_trace_batch(scene.dem, rays, origin=tuple(float(v) for v in scene.origin), spacing=tuple(float(v) for v in scene.spacing),
                                      exaggeration=scene.kw["exaggeration"], inv_two_r_prime=float(scene.inv_two_r_prime),
                                      curvature_enabled=scene.curvature_enabled, any_hit=any_hit, apply_curvature=curved)


def gate_occlusion(ts, curved, hit, what, quiet=False):
    """Occlusion reports a hit exactly when clear <= 0 (a raster bit is set exactly when clear > 0), outside the band."""
    share = ts.conditions(curved)
    want = ts.ref[curved]["clear"] <= 0.0
    wrong = ~ts.band(curved) & (np.asarray(hit, bool) != want)
    if not quiet:
        print(f"trace-ref {ts.name} {what}: {len(want)} rays, {int(want.sum())} occluded, band {100 * share:.3f} %, {int(wrong.sum())} disagree")
    assert 0.05 * len(want) <= want.sum() <= 0.95 * len(want) or ts.raster, f"{ts.name}: {want.mean():.3f} of the rays are occluded"
    assert not wrong.any(), f"{ts.name} {what}: {int(wrong.sum())} rays disagree with the reference, first {np.nonzero(wrong)[0][:5]}"
    return int(wrong.sum())


def measure_closest(ts, hit, t, normal):
    """Hit/miss disagreements outside the band, and over the agreed hits the largest height figure (|f(t)| and how far f dips
    under zero before t, in ulp(max(|o.y|, max height))) and the largest angle to the f64 normal."""
    ref, rays, s = ts.ref[False], ts.rays[False], ts.scene.surface
    want = np.isfinite(ref["first"])
    hit = np.asarray(hit, bool)
    wrong = ~ts.band(False) & (hit != want)
    both = hit & want & ~ts.band(False)
    r, tt = rays[both], np.asarray(t, f32)[both]
    unit = tr.height_unit(s, r)
    residual = np.abs(tr.deviation(s, r, tt))
    dip = np.maximum(-tr.lowest_before(s, r, tt), 0.0)
    height = np.maximum(residual, dip) / unit
    position = r[:, 0:3].astype(f64) + tt.astype(f64)[:, None] * r[:, 4:7].astype(f64)
    angle = tr.normal_angle(s, position, np.asarray(normal, f64)[both])
    return wrong, both, height, angle


def gate_closest(ts, hit, t, normal, what):
    """Closest hit reports a hit exactly when `first` is finite; the hit lies on the surface and nothing was passed under
    before it, both within the height tolerance; the normal within the angle tolerance."""
    share = ts.conditions(False)
    wrong, both, height, angle = measure_closest(ts, hit, t, normal)
    n_hit = int(np.isfinite(ts.ref[False]["first"]).sum())
    print(f"trace-ref {ts.name} {what}: {len(wrong)} rays, {n_hit} hits, band {100 * share:.3f} %, "
          f"height {height.max():.3g} ulp, angle {angle.max():.3g} rad, {int(wrong.sum())} disagree")
    assert 0.05 * len(wrong) <= n_hit <= 0.95 * len(wrong), f"{ts.name}: {n_hit} of {len(wrong)} rays hit"
    assert not wrong.any(), f"{ts.name} {what}: {int(wrong.sum())} rays disagree with the reference, first {np.nonzero(wrong)[0][:5]}"
    assert ts.name in tr.HEIGHT_TOL_ULPS, f"{ts.name}: no measured tolerance in trace_reference.py"
    assert height.max() <= tr.HEIGHT_TOL_ULPS[ts.name], f"{ts.name} {what}: {height.max():.3g} ulp off the surface"
    assert angle.max() <= tr.ANGLE_TOL_RAD[ts.name], f"{ts.name} {what}: normal {angle.max():.3g} rad off"


@pytest.fixture(scope="module")
def world():
    """Every scene and set of this module, the host bodies' scenes included; built once."""
    qlib, rlib = query_lib(), raster_lib()
    made = SimpleNamespace(sets={}, rasters={}, query={}, raster_scene={}, scenes={})
    heights, kw, rays = proof_scene()
    made.query["proof"] = QueryScene(qlib, heights, PROOF_CAM, kw)
    assert made.query["proof"].curvature_enabled and made.query["proof"].inv_two_r_prime > 0.0
    proof = describe(heights, kw, made.query["proof"].inv_two_r_prime)
    assert made.query["proof"].origin == proof.origin
    made.scenes["proof"] = proof
    made.sets["proof"] = TraceSet("proof", proof, rays)
    for i, name in enumerate(SHAPES):
        dem, kw = shape_scene(name)
        made.query[name] = QueryScene(qlib, dem, scenes.CAM, kw)
        made.raster_scene[name] = RasterScene(rlib, dem, kw)
        scene = describe(dem, kw, made.raster_scene[name].inv_two_r_prime)
        assert made.raster_scene[name].origin == scene.origin and made.raster_scene[name].spacing == scene.spacing
        assert made.raster_scene[name].curvature_enabled and f32(made.query[name].inv_two_r_prime) == scene.inv_two_r_prime
        made.scenes[name] = scene
        made.sets[name] = TraceSet(f"list-{name}", scene, list_rays(scene, seed=4100 + i))
        if name in RASTER_SHAPES:
            made.rasters[name] = TraceSet(f"raster-{name}", scene, raster_rays(scene, False), raster=True, rays_curved=raster_rays(scene, True))
    _, _, patched = reterrain_case()  # (the retable path's DEM: a set of its own, measured like the others)
    made.query["64x64-reterrain"] = QueryScene(qlib, patched, scenes.CAM, shape_scene("64x64")[1])
    made.scenes["64x64-reterrain"] = describe(patched, shape_scene("64x64")[1], made.scenes["64x64"].inv_two_r_prime)
    made.sets["64x64-reterrain"] = TraceSet("list-64x64-reterrain", made.scenes["64x64-reterrain"], list_rays(made.scenes["64x64-reterrain"], seed=4242))
    yield made
    for s in list(made.query.values()) + list(made.raster_scene.values()):
        s.close()


LISTS = ["proof"] + list(SHAPES) + ["64x64-reterrain"]


# ---- a. the reference against its brute force -------------------------------------------------------------------------------
def terrace_dem():
    i, j = np.meshgrid(np.arange(24), np.arange(20))
    return (np.floor((i + 0.5 * j) / 4.0) / 6.0 + 0.02 * np.sin(0.9 * i) * (i % 8 < 2)).astype(f32)  # flat cells between risers


def brute_force_cases():
    golden = scenes.golden_dem(4)
    made = []
    for name, dem, spacing, inv in (("golden", golden, (100.0 / 63.0, 100.0 / 63.0), 2e-5), ("terrace", terrace_dem(), (2.0, 3.0), 1e-4),
                                    ("one-cell", np.array([[0.1, 0.9], [0.7, 0.2]], f32), (8.0, 5.0), 1e-3)):
        scene = describe(dem, dict(spacing=spacing, exaggeration=20.0), inv)  # (curvature exaggerated so that the parabola counts)
        s = scene.surface
        rays = list_rays(scene, seed=77, n=14)
        cx, cz, top = 0.5 * (s.X[0] + s.X[-1]), 0.5 * (s.Z[0] + s.Z[-1]), float(s.h64.max())
        extent = s.X[-1] - s.X[0]
        special = np.array([
            [cx + 0.137 * extent, top + 3.0, cz - 0.21 * (s.Z[-1] - s.Z[0]), 1e-3, 0.0, -1.0, 0.0, 2.0 * top + 10.0],   # vertical, down
            [cx - 0.31 * extent, top + 3.0, cz + 0.11 * (s.Z[-1] - s.Z[0]), 1e-3, 0.0, 1.0, 0.0, 50.0],                  # vertical, up
            [s.X[0] - 0.4 * extent, top + 1.0, cz + 0.123, 1e-3, 1.0, -0.02, 0.0371, 1e30],                             # from outside, grazing
            [s.X[-1] + 0.2 * extent, top * 0.9 + 1.0, s.Z[0] - 0.2 * extent, 1e-3, -0.83, -0.05, 0.61, 1e30],           # from outside, across a corner region
            [cx + 0.013, top + 0.5, cz + 0.029, 1e-3, 0.618, -0.07, 0.33, 0.37 * extent],                              # cut by tmax inside a cell
            [cx - 0.2 * extent, top + 0.2, cz, 1e-3, 0.9, 0.001, -0.4358, 1e30],                                       # nearly level: the parabola decides
        ], f32)
        made.append((name, scene, np.concatenate([rays, special])))
    return made


def test_the_reference_equals_its_brute_force():
    total = resolved = 0
    for name, scene, rays in brute_force_cases():
        s = scene.surface
        for curved in (False, True):
            ref = tr.terrain_reference(s, rays, float(scene.inv_two_r_prime), curved)
            for i, ray in enumerate(rays):
                dense = tr.dense_trace(s, ray, float(scene.inv_two_r_prime), curved)
                total += 1
                if dense is None:
                    assert not ref["passes"][i] and ref["clear"][i] == np.inf and ref["first"][i] == np.inf
                    continue
                assert ref["passes"][i]
                # the samples are points of the interval: their minimum is no lower than the true one, and no higher than it
                # by more than f moves between two samples
                assert -1e-9 <= dense["clear"] - ref["clear"][i] <= dense["step"] + 1e-9, (name, curved, i)
                if abs(ref["clear"][i]) <= dense["step"] or dense["starts_under"]:
                    continue  # (a dip the samples may step over, or a start under the surface: nothing to bracket)
                resolved += 1
                lo, hi = dense["bracket"]
                if np.isinf(lo):
                    assert ref["first"][i] == np.inf, (name, curved, i)
                else:
                    assert lo - 1e-9 * abs(lo) <= ref["first"][i] <= hi + 1e-9 * abs(hi), (name, curved, i, lo, ref["first"][i], hi)
                    p = ray[0:3].astype(f64) + ref["first"][i] * ray[4:7].astype(f64)
                    # the normal is that of the surface under the point: central differences of the f64 surface agree
                    h = 1e-6
                    gx = (s.height(p[0] + h, p[2]) - s.height(p[0] - h, p[2])) / (2 * h)
                    gz = (s.height(p[0], p[2] + h) - s.height(p[0], p[2] - h)) / (2 * h)
                    n = np.array([-gx, 1.0, -gz]) / np.sqrt(gx * gx + 1.0 + gz * gz)
                    assert np.arccos(min(1.0, float(n @ ref["normal"][i]))) < 1e-3, (name, curved, i)
    print(f"trace-ref brute force: {total} rays, {resolved} resolved by the dense samples")
    assert total >= 100 and resolved >= 0.8 * total


def test_the_rule_along_a_lattice_line():
    """A ray along a lattice line lies in the cells on the line's higher-index side, and in none along the last line."""
    dem = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], f32)
    scene = describe(dem, dict(spacing=(1.0, 1.0), exaggeration=1.0), 0.0)
    s = scene.surface
    down = lambda x, z: [x, 0.5, z, 0.0, 0.0, -0.2, 1.0, 1e30]
    ref = tr.terrain_reference(s, np.array([down(s.X[1], s.Z[0] - 1.0), down(s.X[2], s.Z[0] - 1.0), down(s.X[0], s.Z[0] - 1.0)], f32))
    assert ref["passes"].tolist() == [True, False, True]
    assert ref["cell"][0].tolist()[0] == 1 and np.isfinite(ref["first"][[0, 2]]).all()


# ---- b. the oracle against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LISTS)
def test_oracle_closest_hit(world, name):
    ts = world.sets[name]
    got = oracle_batch(ts.scene, ts.rays[False], any_hit=False, curved=False)
    gate_closest(ts, got["hit"] != 0, got["t"], got["normal"], "oracle closest")


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("name", LISTS)
def test_oracle_occlusion(world, name, curved):
    ts = world.sets[name]
    gate_occlusion(ts, curved, oracle_batch(ts.scene, ts.rays[curved], any_hit=True, curved=curved)["hit"] != 0, f"oracle occlusion curved={curved}")


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("name", RASTER_SHAPES)
def test_oracle_rasters(world, name, curved):
    ts = world.rasters[name]
    gate_occlusion(ts, curved, oracle_batch(ts.scene, ts.rays[curved], any_hit=True, curved=curved)["hit"] != 0, f"oracle rasters curved={curved}")


def test_measured_tolerances_are_four_times_the_oracles_maxima(world):
    """The constants of trace_reference.py against a fresh measurement: each recorded maximum is the oracle's (to the two
    digits it is written with, rounded up), and the gates are four times that."""
    for name in LISTS:
        ts = world.sets[name]
        got = oracle_batch(ts.scene, ts.rays[False], any_hit=False, curved=False)
        _, _, height, angle = measure_closest(ts, got["hit"] != 0, got["t"], got["normal"])
        recorded = tr.MEASURED_ON_THE_ORACLE[ts.name]
        print(f"trace-ref measured {ts.name!r}: ({height.max():.4g}, {angle.max():.4g}),")
        assert height.max() <= recorded[0] <= 1.05 * height.max() + 0.01 and angle.max() <= recorded[1] <= 1.05 * angle.max() + 1e-9
        assert tr.HEIGHT_TOL_ULPS[ts.name] == 4.0 * recorded[0] and tr.ANGLE_TOL_RAD[ts.name] == 4.0 * recorded[1]


# ---- c. the host lane bodies against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", LISTS)
def test_query_body_closest_hit(world, name):
    ts = world.sets[name]
    got = world.query[name].run(0, ts.rays[False])
    assert not (got["kind"] == 2).any()
    gate_closest(ts, got["kind"] == 1, got["t"], got["normal"], "query body closest")
    hit = got["kind"] == 1
    want = ts.rays[False][hit, 0:3].astype(f64) + got["t"][hit].astype(f64)[:, None] * ts.rays[False][hit, 4:7].astype(f64)
    scale = np.maximum(np.abs(want).max(axis=1), 1.0)
    assert (np.abs(got["position"][hit] - want).max(axis=1) <= 4 * np.spacing(f32(1.0)) * scale).all(), "position is o + t d"


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("name", LISTS)
def test_query_body_occlusion(world, name, curved):
    ts = world.sets[name]
    got = world.query[name].run(1, ts.rays[curved], flags=2 if curved else 0)
    gate_occlusion(ts, curved, got["kind"] != 0, f"query body occlusion curved={curved}")


@pytest.mark.parametrize("mode", [2, 3, 6, 7])
@pytest.mark.parametrize("name", LISTS)
def test_emulator_march(world, name, mode):
    """The stackless march: 2 any hit, 3 closest, +4 started in the cell under the origin."""
    ts = world.sets[name]
    sc = ts.scene
    for curved in ((False, True) if mode & 3 == 2 else (False,)):
        got = emul.terrain_trace_batch(sc.dem, ts.rays[curved], origin=tuple(float(v) for v in sc.origin), spacing=tuple(float(v) for v in sc.spacing),
                                       exaggeration=sc.kw["exaggeration"], inv_two_r_prime=float(sc.inv_two_r_prime), curvature_enabled=True,
                                       any_hit=mode, apply_curvature=curved)
        if mode & 3 == 2:
            gate_occlusion(ts, curved, got["hit"] != 0, f"march mode {mode} curved={curved}")
        else:
            gate_closest(ts, got["hit"] != 0, got["t"], got["normal"], f"march mode {mode}")


def raster_bits(scene, run, curved):
    """The bits of raster_rays' rasters, in its order, from `run(mode, targets, lift) -> bool (K, rows, cols)`; only the
    samples that march."""
    observers, _ = viewshed_targets(scene, 2)
    suns = np.stack([sun_direction(az, el) for az, el in SUNS])
    region = (0, 0, *scene.dem.shape)
    out = []
    for lift in LIFTS:
        o = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, region, lift)
        for mode, targets in ((TOWARD, observers), (ALONG, suns)):
            masks = run(mode, targets, lift)
            for target, mask in zip(targets, masks):
                _, go = contract_rays(o, mode, target, curved, scene.inv_two_r_prime, scene.curvature_enabled)
                assert not np.asarray(mask).reshape(-1)[~go].any(), "cut off by the distance limit: not visible"
                out.append(np.asarray(mask).reshape(-1)[go])
    return np.concatenate(out)


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("name", RASTER_SHAPES)
def test_raster_body(world, name, curved):
    ts = world.rasters[name]
    host = world.raster_scene[name]
    lit = raster_bits(ts.scene, lambda mode, targets, lift: host.run(mode, targets, flags=CURVED if curved else 0, lift=lift)["masks"], curved)
    assert len(lit) == len(ts.rays[curved])
    gate_occlusion(ts, curved, ~lit, f"raster body curved={curved}")
    assert lit.any() and (ts.ref[curved]["clear"].min() > 0.0 or not lit.all())


def test_whitebox_curved_viewshed_on_the_raster_body():
    """The reference's curved-earth golden scene (a flat 256x256 DEM, 111 km across, the observer 250 m up): here the curvature
    term alone decides, and a wrong sign of it in the sight lines or in the march flips thousands of bits.  The flat DEM has no
    relief, so the band is empty: every bit of the raster body equals the f64 reference's."""
    from test_session_raster_host import iou, whitebox_observer, whitebox_reference, whitebox_scene_kwargs

    dem, kw = whitebox_scene_kwargs()
    host = RasterScene(raster_lib(), dem, kw, cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        scene = describe(dem, kw, host.inv_two_r_prime)
        assert host.origin == scene.origin and host.spacing == scene.spacing and host.curvature_enabled
        obs = whitebox_observer(scene.origin, scene.spacing)
        o = contract_origins(dem, kw["exaggeration"], scene.origin, scene.spacing, (0, 0, *dem.shape), f32(1e-3))
        rays, go = contract_rays(o, TOWARD, obs[0], True, scene.inv_two_r_prime, True)
        assert go.all()
        ts = TraceSet("raster-whitebox", scene, rays, raster=True, which=(True,))
        lit = host.run(TOWARD, obs, flags=CURVED, lift=1e-3)["masks"][0]
        gate_occlusion(ts, True, ~lit.reshape(-1), "raster body curved=True")
        reference = (ts.ref[True]["clear"] > 0.0).reshape(dem.shape)
        print(f"whitebox golden: the f64 reference's own IoU {iou(reference, whitebox_reference()):.5f} ({int(reference.sum())} visible)")
        assert 0.1 * lit.size < (~lit).sum() < 0.9 * lit.size, "the horizon cuts the raster"
    finally:
        host.close()


# ---- the box city: terrain OR triangles --------------------------------------------------------------------------------------
def city_scene():
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    assert len(tris) == 385
    return dem, verts, tris, _kw(dem, mesh_vertices=verts, mesh_indices=tris)


def city_raster_targets(scene):
    """One observer and one generic sun over the city (lift 1e-3): (mode, targets (1, 4)) pairs."""
    return [(TOWARD, viewshed_targets(scene, 1)[0]), (ALONG, sun_direction(*SUNS[1])[None, :])]


def city_raster_rays(scene, curved):
    o = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, (0, 0, *scene.dem.shape), 1e-3)
    out = []
    for mode, targets in city_raster_targets(scene):
        rays, go = contract_rays(o, mode, targets[0], curved, scene.inv_two_r_prime, scene.curvature_enabled)
        assert go.all()
        out.append(rays)
    return np.concatenate(out)


class CitySets:
    """The list rays and the raster rays over the city with both references' answers (the mesh is met by the straight ray:
    the curvature policy bends the terrain test only)."""

    def __init__(self, scene, verts, tris):
        self.list = TraceSet("list-64x64", scene, list_rays(scene, seed=4177))
        self.raster = TraceSet("raster-city", scene, city_raster_rays(scene, False), raster=True, rays_curved=city_raster_rays(scene, True))
        self.mesh = {(ts.name, curved): tr.mesh_reference(verts, tris, ts.rays[curved]) for ts in (self.list, self.raster) for curved in (False, True)}


def gate_city(ts, mesh, curved, hit, terrain_only, what):
    """Occluded exactly when the terrain reference OR the f64 triangle search says so; left out: the terrain's band and rays
    whose barycentric margin is under 1e-6 (at most 1 % of the set)."""
    if terrain_only:
        return gate_occlusion(ts, curved, hit, what)
    share = ts.conditions(curved)
    edge = mesh["margin"] < tr.MESH_BAND
    assert edge.mean() <= tr.MESH_BAND_CAP, f"{ts.name}: {100 * edge.mean():.2f} % of the rays graze a triangle's edge"
    blocked = np.isfinite(mesh["t"])
    want = (ts.ref[curved]["clear"] <= 0.0) | blocked
    wrong = ~edge & ~(ts.band(curved) & ~blocked) & (np.asarray(hit, bool) != want)
    print(f"trace-ref {ts.name} {what}: {len(want)} rays, {int(want.sum())} occluded ({int(blocked.sum())} by the mesh), band {100 * share:.3f} %, "
          f"edge band {100 * edge.mean():.3f} %, {int(wrong.sum())} disagree")
    assert blocked.sum() > 0.02 * len(want), "the boxes block rays"
    assert not wrong.any(), f"{ts.name} {what}: {int(wrong.sum())} rays disagree with the references, first {np.nonzero(wrong)[0][:5]}"
    return int(wrong.sum())


@pytest.fixture(scope="module")
def city(world):
    dem, verts, tris, kw = city_scene()
    scene = world.scenes["64x64"]
    assert np.array_equal(scene.dem, dem)
    return dem, kw, CitySets(scene, verts, tris)


@pytest.mark.parametrize("mesh_form", [0, 1, 2])
def test_city_on_the_host_bodies(city, mesh_form):
    dem, kw, sets = city
    query = QueryScene(query_lib(), dem, scenes.CAM, kw, mesh_form=mesh_form)
    raster = RasterScene(raster_lib(), dem, kw, mesh_form=mesh_form)
    try:
        for curved in (False, True):
            for terrain_only in (False, True):
                flags = (2 if curved else 0) | (1 if terrain_only else 0)
                got = query.run(1, sets.list.rays[curved], flags=flags)["kind"] != 0
                gate_city(sets.list, sets.mesh["list-64x64", curved], curved, got, terrain_only, f"city query body curved={curved} terrain_only={terrain_only}")
                lit = np.concatenate([raster.run(mode, targets, flags=flags, lift=1e-3)["masks"].reshape(-1) for mode, targets in city_raster_targets(sets.raster.scene)])
                gate_city(sets.raster, sets.mesh["raster-city", curved], curved, ~lit, terrain_only, f"city raster body curved={curved} terrain_only={terrain_only}")
    finally:
        query.close()
        raster.close()


# ---- the mesh search ----------------------------------------------------------------------------------------------------------
def test_triangle_search_on_known_triangles():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0], [1, 1, 0], [0, 1, 1]], f32)
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    rays = np.array([[0.25, 2.0, 0.25, 1e-3, 0, -1, 0, 1e30], [0.25, 2.0, 0.25, 1e-3, 0, -1, 0, 1.5], [0.9, 2.0, 0.9, 1e-3, 0, -1, 0, 1e30],
                     [0.5, 2.0, 1e-7, 1e-3, 0, -1, 0, 1e30]], f32)
    got = tr.mesh_reference(verts, tris, rays)
    assert np.allclose(got["t"][[0, 1, 3]], [1.0, 1.0, 1.0]) and got["t"][2] == np.inf
    assert got["triangle"].tolist() == [1, 1, -1, 1]
    assert abs(got["margin"][0] - 0.25) < 1e-6 and got["margin"][2] == np.inf and got["margin"][3] < 1e-6
