"""The bits of the raster lane bodies on stored inputs -- TEST INFRASTRUCTURE ONLY.

What tests/golden/make_walk_bits.py (the generator of tests/golden/raster_walk_bits.npz), tests/test_walk_bits_host.py and
tests/test_gpu_walk_bits.py share: the shapes, the inputs as the generator makes them, the host harnesses of a checkout, and
the cases -- every (key, plane) a set of inputs yields on the host, and the keys of those the library can be asked for.

A key is "family/ROWSxCOLS/flat|curved/rows|block/case/plane".  The float64 references are not here: this pins bits.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

import scenes
from emul import emul
from test_session_raster_host import _kw, shaped_dem
from test_session_rearm_host import _desc

f32 = np.float32
SIZE = (96, 64)
SHAPES = [(2, 2), (2, 9), (9, 2), (3, 5), (33, 33), (63, 65)]  # (rows, cols)
REGIONS = {(63, 65): [(1, 2, 2, 3), (62, 64, 1, 1)]}  # windows, besides the whole DEM
FULL_PLANES_UP_TO = 18  # samples: the shapes whose planes the fixture holds in full
TINY_CAP = 3
CURVED, SESSION_SUN, HORIZONTAL = 2, 16, 16
HARNESSES = {"horizon": "horizon_host/horizon_harness.cpp", "clearance": "clearance_host/clearance_harness.cpp",
             "umbra": "umbra_host/umbra_harness.cpp", "raster": "raster_host/raster_harness.cpp",
             "irradiation": "irradiation_host/irradiation_harness.cpp"}


def shape_name(shape):
    return f"{shape[0]}x{shape[1]}"


def digest(plane) -> str:
    return hashlib.sha256(np.ascontiguousarray(plane).astype("<f4", copy=False).tobytes()).hexdigest()


def plane_at(origin, index, spacing):
    """f3d_trace.h plane_at: fma(f32(index), spacing, origin)."""
    return f32(np.float64(index) * np.float64(spacing) + np.float64(origin))


# ---- the inputs (the generator's; the tests read them from the fixture) -----------------------------------------------------------
def horizon_azimuths():
    from forge3d_amd.session import TerrainSession

    odd = [(3, -1.5), (-0.7, 2.2), (0, -4), (5, 0), (1, 1), (-1, 1), (-2, -2), (1e-3, 5e-4)]
    return np.concatenate([np.asarray(TerrainSession.horizon_directions(16), f32).reshape(16, 2), np.array(odd, f32)])


HORIZON_LIFTS = np.array([0.0, 1e-3, 0.5], f32)

UMBRA_DIRECTIONS = np.array([
    (-0.70, 0.09, -0.70, 0), (0.55, 0.50, -0.66, 0),  # dy > 0
    (-0.8, 0.0, 0.6, 0),                              # dy == 0
    (0.6, -0.05, 0.8, 0),                             # dy < 0
    (1.0, 0.17, 0.0, 0), (0.0, 0.34, -1.0, 0),        # the flat axes
    (1.0, 0.2, 1.0, 0), (-1.0, 0.1, 1.0, 0), (-2.0, 0.3, -2.0, 0),  # through lattice corners (square spacing)
    (0.0, 1.0, 0.0, 0), (0.0, -1.0, 0.0, 0),          # straight up, straight down: no walk
], f32)


def clearance_observers(dem, exaggeration, origin, spacing):
    """(K, 4) f32 for one DEM: see the comments."""
    rows, cols = dem.shape
    held = np.asarray(dem, f32) * f32(exaggeration)
    top, low = float(held.max()), float(held.min())
    high = top + 0.25 * (top - low) + 1.0
    ic, jc = (cols - 1) // 2, (rows - 1) // 2
    x_on, z_on = float(plane_at(origin[0], ic, spacing[0])), float(plane_at(origin[1], jc, spacing[1]))
    x_in, z_in = x_on + 0.37 * float(spacing[0]), z_on + 0.21 * float(spacing[1])
    x0, x1 = float(plane_at(origin[0], 0, spacing[0])), float(plane_at(origin[0], cols - 1, spacing[0]))
    z0, z1 = float(plane_at(origin[1], 0, spacing[1])), float(plane_at(origin[1], rows - 1, spacing[1]))
    out_x, out_z = 0.8 * float(spacing[0]) + 0.3 * (x1 - x0), 0.6 * float(spacing[1]) + 0.3 * (z1 - z0)
    span = float(np.hypot(x1 - x0, z1 - z0))
    return np.array([
        (x_in, high, z_in, 0),            # above the centre, inside a cell
        (x_on, high, z_on, 0),            # exactly on a lattice point: hd2 == 0 for one sample
        (x_on, high, z_in, 0),            # on a lattice line: a flat x axis for a whole column
        (x_in, high, z_on, 0),            # ... a flat z axis for a whole row
        (x0 - out_x, high, z_in, 0), (x1 + out_x, high, z_in, 0),  # outside the footprint on each side
        (x_in, high, z0 - out_z, 0), (x_in, high, z1 + out_z, 0),
        (x1 + out_x, high, z1 + out_z, 0),  # ... and off a corner
        (x_in, low - 10.0, z_in, 0),      # under the surface: the +inf leaf exit
        (x_in, high, z_in, 0.35 * span),  # a distance limit that cuts the raster
    ], f32)


def make_inputs(harnesses):
    """The fixture's input arrays, from the scenes as `harnesses` sets them up."""
    inputs = {"horizon_azimuths": horizon_azimuths(), "horizon_lifts": HORIZON_LIFTS, "umbra_directions": UMBRA_DIRECTIONS,
              "irradiation_directions": np.array([(-0.5, 0.6, -0.62, 1.0)], f32), "raster_targets": np.array([(-0.7, 0.26, -0.66, 0)], f32)}
    for shape in SHAPES:
        dem = shaped_dem(shape)
        kw = _kw(dem)
        scene = Scene(harnesses, "clearance", dem, kw)
        inputs[f"clearance_observers_{shape_name(shape)}"] = clearance_observers(dem, kw["exaggeration"], scene.info[0:2], scene.info[2:4])
        scene.close()
    return inputs


# ---- the host harnesses of a checkout --------------------------------------------------------------------------------------------
def build_harnesses(root: Path) -> dict:
    """The five raster harnesses of the checkout at `root`, built with emul.CXX (side by side) and loaded."""
    out = Path(tempfile.mkdtemp(prefix="f3d_walk_bits_"))

    def one(item):
        name, source = item
        lib = out / f"lib{name}.so"
        subprocess.run([*emul.CXX, str(Path(root) / "tests" / source), "-o", str(lib)], check=True, capture_output=True)
        return name, C.CDLL(str(lib))

    with ThreadPoolExecutor(len(HARNESSES)) as pool:
        libs = dict(pool.map(one, HARNESSES.items()))
    u32, ptr, flt = C.c_uint32, C.c_void_p, C.c_float
    for name, lib in libs.items():
        create = getattr(lib, f"{name}_scene_create")
        create.restype = ptr
        create.argtypes = [ptr, C.c_int32, ptr] if name in ("raster", "irradiation") else [ptr, ptr]
        getattr(lib, f"{name}_scene_destroy").argtypes = [ptr]
        getattr(lib, f"{name}_run").restype = C.c_int
    libs["horizon"].horizon_run.argtypes = [ptr] + [u32] * 5 + [flt, u32] + [ptr] * 4 + [u32] * 2
    libs["clearance"].clearance_run.argtypes = [ptr] + [u32] * 6 + [ptr] * 4 + [u32] * 2
    libs["umbra"].umbra_run.argtypes = [ptr] + [u32] * 6 + [ptr] * 4 + [u32] * 2
    libs["raster"].raster_run.argtypes = [ptr] + [u32] * 6 + [flt, u32] + [ptr] * 5
    libs["irradiation"].irradiation_run.argtypes = [ptr] + [u32] * 5 + [flt, u32] + [ptr] * 6
    return libs


class Scene:
    """A scene as one family's harness sets it up."""

    def __init__(self, harnesses, family, dem, kw):
        self.lib, self.family, self.dem = harnesses[family], family, np.ascontiguousarray(dem, f32)
        d, keep = _desc(self.dem, SIZE, scenes.CAM, kw)
        self.info = np.zeros(9, f32)
        create = getattr(self.lib, f"{family}_scene_create")
        args = (C.addressof(d), 2, self.info.ctypes.data) if family in ("raster", "irradiation") else (C.addressof(d), self.info.ctypes.data)
        self.handle = create(*args)
        del keep
        assert self.handle, "the scene's descriptor was refused"

    def close(self):
        getattr(self.lib, f"{self.family}_scene_destroy")(self.handle)


def _p(a):
    return a.ctypes.data


def _horizon(s, flags, region, lift, az, cap, block):
    n, k = region[2] * region[3], len(az)
    h, sky, o = np.empty((k, n), f32), np.empty(n, f32), np.empty((n, 3), f32)
    assert s.lib.horizon_run(s.handle, flags, *region, float(lift), k, _p(az), _p(h), _p(sky), _p(o), cap, block) == 0
    return {"horizon": h, "sky_view": sky, "origins": o}


def _clearance(s, flags, region, obs, cap, block):
    n, k = region[2] * region[3], len(obs)
    h, low, o = np.empty((k, n), f32), np.empty(n, f32), np.empty((n, 3), f32)
    assert s.lib.clearance_run(s.handle, flags, *region, k, _p(obs), _p(h), _p(low), _p(o), cap, block) == 0
    return {"height": h, "lowest": low, "origins": o}


def _umbra(s, flags, region, dirs, cap, block):
    n, k = region[2] * region[3], 1 if dirs is None else len(dirs)
    d, deep, o = np.empty((k, n), f32), np.empty(n, f32), np.empty((n, 3), f32)
    assert s.lib.umbra_run(s.handle, flags | (SESSION_SUN if dirs is None else 0), *region, k, None if dirs is None else _p(dirs),
                           _p(d), _p(deep), _p(o), cap, block) == 0
    return {"depth": d, "deepest": deep, "origins": o}


def regions_of(shape):
    return [("whole", (0, 0, *shape))] + [("r" + "_".join(map(str, r)), r) for r in REGIONS.get(shape, [])]


def host_cases(harnesses, inputs, shape):
    """Every (key, f32 plane) of one shape on the host harnesses."""
    dem = shaped_dem(shape)
    kw = _kw(dem)
    az, dirs = np.ascontiguousarray(inputs["horizon_azimuths"], f32), np.ascontiguousarray(inputs["umbra_directions"], f32)
    obs = np.ascontiguousarray(inputs[f"clearance_observers_{shape_name(shape)}"], f32)
    sn = shape_name(shape)
    for family in ("horizon", "clearance", "umbra"):
        s = Scene(harnesses, family, dem, kw)
        for curved in (0, CURVED):
            for block in (0, 1):
                head = f"{family}/{sn}/{'curved' if curved else 'flat'}/{'block' if block else 'rows'}"
                for rname, region in regions_of(shape):
                    runs = {}
                    if family == "horizon":
                        for lift in inputs["horizon_lifts"]:
                            runs[f"{rname}_lift{float(lift):g}"] = _horizon(s, curved, region, lift, az, 0, block)
                        if rname == "whole":
                            runs["cap"] = _horizon(s, curved, region, 1e-3, az, TINY_CAP, block)
                    elif family == "clearance":
                        runs[rname] = _clearance(s, curved, region, obs, 0, block)
                        if rname == "whole":
                            runs["cap"] = _clearance(s, curved, region, obs, TINY_CAP, block)
                    else:
                        runs[rname] = _umbra(s, curved, region, dirs, 0, block)
                        runs[f"{rname}_sun"] = _umbra(s, curved, region, None, 0, block)
                        if rname == "whole":
                            runs["cap"] = _umbra(s, curved, region, dirs, TINY_CAP, block)
                    for case, planes in runs.items():
                        for name, plane in planes.items():
                            yield f"{head}/{case}/{name}", plane
        s.close()
    # the lattice points (and what else the changed origin functions feed) of the two marching families
    targets, terms = np.ascontiguousarray(inputs["raster_targets"], f32), np.ascontiguousarray(inputs["irradiation_directions"], f32)
    s = Scene(harnesses, "raster", dem, kw)
    for rname, region in regions_of(shape):
        for lift in inputs["horizon_lifts"]:
            n = region[2] * region[3]
            o = np.empty((n, 3), f32)
            assert s.lib.raster_run(s.handle, 1, 1, *region, float(lift), 1, _p(targets), None, None, None, _p(o)) == 0
            yield f"raster/{sn}/flat/rows/{rname}_lift{float(lift):g}/origins", o
    s.close()
    s = Scene(harnesses, "irradiation", dem, kw)
    for rname, region in regions_of(shape):
        for lift in inputs["horizon_lifts"]:
            n = region[2] * region[3]
            o, energy, normal = np.empty((n, 3), f32), np.empty(n, f32), np.empty((n, 3), f32)
            assert s.lib.irradiation_run(s.handle, 1, *region, float(lift), 1, _p(terms), _p(energy), None, _p(normal), None, _p(o)) == 0
            for name, plane in (("origins", o), ("energy", energy), ("normal", normal)):
                yield f"irradiation/{sn}/flat/rows/{rname}_lift{float(lift):g}/{name}", plane
    s.close()


def stored_key(key):
    """The key a plane's digest is stored under: the two wave footprints own the same samples and share one."""
    return key.replace("/block/", "/rows/")


class Fixture:
    """tests/golden/raster_walk_bits.npz: `inputs` (what make_inputs made), `want` (key -> hex digest), `planes` (key -> the
    plane, flat, for the small DEMs)."""

    def __init__(self, path):
        with np.load(path) as z:
            self.inputs = {k: z[k] for k in z.files}
        self.commit = str(self.inputs["commit"])
        self.want = {str(k): bytes(d).hex() for k, d in zip(self.inputs["keys"], self.inputs["digests"])}
        starts, flat = self.inputs["plane_starts"], self.inputs["planes"]
        self.planes = {str(k): flat[starts[n]:starts[n + 1]] for n, k in enumerate(self.inputs["plane_keys"])}

    def mismatch(self, key, plane):
        """None when `plane` has the stored bits of `key`, else what to report."""
        if digest(plane) == self.want[stored_key(key)]:
            return None
        family, shape, curved, footprint, case, name = key.split("/")
        stored = self.planes.get(stored_key(key))
        where = "" if stored is None else f"; first differing sample {first_difference(plane, stored)} of\n{np.asarray(plane).ravel()}\nstored\n{stored}"
        return f"{family} {name}, case {case}, {curved}, footprint {footprint}, DEM {shape}: not the bits of {self.commit[:7]}{where}"


def first_difference(got, want):
    """Index of the first sample whose bits differ (flat index into the plane)."""
    a, b = np.asarray(got, f32).ravel().view(np.uint32), np.asarray(want, f32).ravel().view(np.uint32)
    return int(np.flatnonzero(a != b)[0]) if a.shape == b.shape and (a != b).any() else -1


# ---- the same inputs through the library (the cases it can express: no injected cap) --------------------------------------------
def device_cases(session, inputs, shape):
    """Every (key, f32 plane) of one shape through f3d_session_horizon / _clearance / _umbra on `session`.  The library picks
    the wave footprint itself; the keys are the "rows" ones (the fixture's generator checks that "block" holds the same bits)."""
    az, dirs = np.ascontiguousarray(inputs["horizon_azimuths"], f32), np.ascontiguousarray(inputs["umbra_directions"], f32)
    obs = np.ascontiguousarray(inputs[f"clearance_observers_{shape_name(shape)}"], f32)
    sn = shape_name(shape)
    for curved in (False, True):
        for rname, region in regions_of(shape):
            how = dict(curved=curved, region=region)
            tail = f"{sn}/{'curved' if curved else 'flat'}/rows"
            for lift in inputs["horizon_lifts"]:
                h, sky = session.horizon(az, lift=float(lift), sky_view=True, **how)
                yield f"horizon/{tail}/{rname}_lift{float(lift):g}/horizon", h
                yield f"horizon/{tail}/{rname}_lift{float(lift):g}/sky_view", sky
            h, low = session.clearance(obs, lowest=True, **how)
            yield f"clearance/{tail}/{rname}/height", h
            yield f"clearance/{tail}/{rname}/lowest", low
            d, deep = session.umbra(dirs, deepest=True, **how)
            yield f"umbra/{tail}/{rname}/depth", d
            yield f"umbra/{tail}/{rname}/deepest", deep
            d, deep = session.umbra(None, deepest=True, **how)
            yield f"umbra/{tail}/{rname}_sun/depth", d
            yield f"umbra/{tail}/{rname}_sun/deepest", deep
