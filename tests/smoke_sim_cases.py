"""Inputs shared by the smoke solver's tests (test_smoke_sim.py, test_smoke_sim_reference_host.py,
test_gpu_smoke_sim_reference.py): the grids that reach the drivers' limits, and the sets the float64 reference
(smoke_sim_reference.py) is compared on.  Plain data and seeded arrays: nothing here runs a solver."""
from __future__ import annotations

import functools

import numpy as np

REFERENCE_THRESHOLD = 1.0e-3  # sparse_threshold of the reference sets: the age band then lies clear of both empty air and smoke

# ---- grids that reach the limits of csrc/f3d_smoke_sim.hip, (nx, ny, nz), each named for what it reaches ---------------------
EDGE_GRIDS = {
    "no-interior": (2, 2, 2),          # no interior voxel; eight voxels; one workgroup in the persistent form
    "one-interior": (3, 3, 3),         # one interior voxel; the confinement's margin-2 interior is empty
    "first-margin2": (5, 5, 5),        # the first grid where the margin-2 interior has a voxel
    "x-flat": (2, 5, 3),               # one axis without interior
    "y-flat": (7, 2, 5),
    "one-tile": (96, 8, 4),            # exactly one Jacobi tile; the one-voxel x halo at full tile width
    "tile-plus-one": (97, 9, 5),       # one voxel into a second tile on every axis; the K-voxel x halo; ragged tiles
    "three-tiles": (193, 3, 3),        # three tiles in x, the middle one with both x halos inside the grid; y, z under a tile
    "slab-second-row": (5, 65, 3),     # ny > 64: the slab sum's lanes take a second row
    "total-second-trip": (3, 3, 65),   # four sum kinds x nz = 260 > 256: the total's copy loop takes a second trip
    "slab-lds-max": (115, 128, 2),     # the slab staging at 61 388 bytes of dynamic LDS, the largest the driver allows
    "slab-lds-over": (116, 128, 2),    # the first grid over that limit: the driver chooses the row form by itself
}
EDGE_SETTINGS = dict(dt=0.1, turbulence_strength=0.8, turbulence_seed=31, wind=(1.2, 0.05, -0.7), velocity_damping=0.05, boundary_damping=0.2,
                     mac_cormack=True, diffusion=0.01, vorticity=0.4, pressure_iterations=7)  # tiled: launches of 4 + 3, then 3
EDGE_NINE_SWEEPS = "tile-plus-one"     # ... also with 9 iterations: 4 + 4 + 1, then 4
EDGE_EMITTERS = [dict(center=(1.0, 1.0, 1.0), radius=3.0)]
EDGE_STEPS = 2


def edge_cases():
    """name -> (geometry, emitters, settings, steps)"""
    out = {name: (dict(dims=dims), EDGE_EMITTERS, dict(EDGE_SETTINGS), EDGE_STEPS) for name, dims in EDGE_GRIDS.items()}
    out[EDGE_NINE_SWEEPS + "-9"] = (dict(dims=EDGE_GRIDS[EDGE_NINE_SWEEPS]), EDGE_EMITTERS, dict(EDGE_SETTINGS, pressure_iterations=9), EDGE_STEPS)
    return out


def seed_edge(fields, seed=5):
    """Seeded velocity, humidity and density into a mapping or object of float32 (nz, ny, nx[, 3]) arrays."""
    rng = np.random.default_rng(seed)
    get, put = _access(fields)
    put("velocity", rng.normal(scale=1.0, size=get("velocity").shape).astype(np.float32))
    put("humidity", (rng.random(get("humidity").shape).astype(np.float32) * np.float32(0.1)).astype(np.float32))
    put("density", (np.float32(1.0) + rng.random(get("density").shape).astype(np.float32) * np.float32(0.5)).astype(np.float32))


def seed_run(fields, seed=3):
    """The initial state of test_smoke_sim._run: a normal velocity and some humidity."""
    rng = np.random.default_rng(seed)
    get, put = _access(fields)
    put("velocity", rng.normal(scale=0.2, size=get("velocity").shape).astype(np.float32))
    put("humidity", (rng.random(get("humidity").shape).astype(np.float32) * np.float32(0.1)).astype(np.float32))


def seed_aged(fields, seed=7):
    """Old smoke: patches of density with ages up to 40 s, so that the age-dependent decay (its ramp runs from 7 to 36 s) and the
    sub-grid eddies' ageing (2 to 28 s) take part -- the steps of the other sets never get older than a second."""
    rng = np.random.default_rng(seed)
    get, put = _access(fields)
    shape = get("density").shape
    put("velocity", rng.normal(scale=0.5, size=shape + (3,)).astype(np.float32))
    put("humidity", (rng.random(shape).astype(np.float32) * np.float32(0.1)).astype(np.float32))
    density = np.where(rng.random(shape) < 0.7, rng.random(shape) * 1.5 + 0.1, 0.0).astype(np.float32)
    put("density", density)
    put("soot", (density * np.float32(0.3)).astype(np.float32))
    put("fuel", (density * np.float32(0.2)).astype(np.float32))
    put("temperature", (rng.random(shape).astype(np.float32) * np.float32(0.5)).astype(np.float32))
    put("particle_age", np.where(density > 0.0, rng.random(shape) * 40.0, -1.0).astype(np.float32))


def _access(fields):
    if isinstance(fields, dict):
        return fields.__getitem__, fields.__setitem__
    return (lambda k: getattr(fields, k)), (lambda k, v: setattr(fields, k, v))


# ---- the sets of the float64 reference ---------------------------------------------------------------------------------------
_PLUME = [dict(center=(9.0, 4.0, 11.0), radius=3.0, density_rate=6.0, temperature_rate=5.0, soot_rate=0.6, humidity_rate=0.3, fuel_rate=0.5,
               velocity=(0.4, 1.5, 0.1))]
_BARE = dict(dt=0.2, turbulence_strength=0.0, vorticity=0.0, diffusion=0.0, velocity_damping=0.0, mac_cormack=False, mass_conservation=False,
             pressure_iterations=1)
_BARE_GRID = dict(dims=(20, 14, 18))
_BARE_STEPS = 3
_PLUS_ONE = {
    "turbulence-wind": dict(turbulence_strength=0.8, turbulence_seed=31, wind=(1.2, 0.05, -0.7)),
    "turbulence-calm": dict(turbulence_strength=0.8, turbulence_seed=31),
    "vorticity": dict(vorticity=0.4),
    "diffusion": dict(diffusion=0.01),
    "maccormack": dict(mac_cormack=True),
    "mass": dict(mass_conservation=True),
    "damping": dict(velocity_damping=0.05),
    "pressure30": dict(pressure_iterations=30),
}
REFERENCE_EDGES = ("one-interior", "first-margin2", "tile-plus-one")  # the edge grids the device is also held to the reference on
# Seeds, chosen so that the reference ALONE leaves out less than its cap of voxels (smoke_sim_reference.BAND_CAP; the tests assert
# it).  The MacCormack band holds 0.6-1.2 % of a 18^3 grid whose back-traces are a few hundredths of a voxel long (three axes x
# 2e-4 voxel x the displacements' density at 0), so "case-maccormack" takes a seed from the lower half of that spread.
_SEEDS = {"case-maccormack": 5}


def reference_sets():
    """name -> (geometry, emitters, settings, steps, seeder): the six cases of test_smoke_sim.py, a bare configuration, the
    bare configuration with exactly one pass turned on each (a failure names its pass), old smoke with every pass on, and three
    edge grids.  Every set runs
    at sparse_threshold = REFERENCE_THRESHOLD."""
    from test_smoke_sim import _cases

    out = {"case-" + name: (geo, em, st, steps, functools.partial(seed_run, seed=_SEEDS.get("case-" + name, 3)))
           for name, (geo, em, st, steps) in _cases().items()}
    out["bare"] = (_BARE_GRID, _PLUME, dict(_BARE), _BARE_STEPS, seed_run)
    for name, extra in _PLUS_ONE.items():
        out["bare+" + name] = (_BARE_GRID, _PLUME, dict(_BARE, **extra), _BARE_STEPS, seed_run)
    out["bare+voxel"] = (dict(dims=(20, 14, 18), voxel_size=(1.5, 1.0, 2.0), origin=(-3.0, 0.0, 2.0)), _PLUME, dict(_BARE), _BARE_STEPS, seed_run)
    # (without MacCormack: thin smoke on a wall gets a lane-shear push of ~1e-5 voxel off the wall, which is the clamp's band)
    out["aged"] = (_BARE_GRID, _PLUME, dict(EDGE_SETTINGS, density_decay=0.5, mac_cormack=False), 2, seed_aged)
    edges = edge_cases()
    for name in REFERENCE_EDGES:
        geo, em, st, steps = edges[name]
        out["edge-" + name] = (geo, em, st, steps, seed_edge)
    return out
