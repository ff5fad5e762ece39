"""Inputs of the smoke ray-marcher's tests -- TEST INFRASTRUCTURE ONLY.

`reference_sets()`: the named sets that tests/test_smoke_march_reference_host.py (oracle) and
tests/test_gpu_smoke_march_reference.py (device) hold to the float64 statement of a ray (tests/smoke_march_reference.py), each
chosen for the branch of the shading it reaches.  Grids are no larger than 24 x 16 x 20 and images no larger than 48 x 36, so a
reference image is a fraction of a second of NumPy.  A set is one render: the `projection*` sets are the map-aligned render,
all others the perspective one.  Beyond the sets the issue names there is `tiny-voxel`: voxel edges under 1e-4, so that the default
step is its floor (the only way to see that constant).

`case(seed)`: the seeded random scene of tools/gpu_fuzz_smoke.py, which the tool and the fuzz slice of tests/test_smoke.py
share."""
from __future__ import annotations

import numpy as np

SUN = (0.4, 0.8, -0.2)


def ball(dims, centre, radius, value):
    nz, ny, nx = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.sqrt((x + 0.5 - centre[0]) ** 2 + (y + 0.5 - centre[1]) ** 2 + (z + 0.5 - centre[2]) ** 2)
    t = np.clip(d / radius, 0.0, 1.0)
    return (value * (1.0 - t * t * (3.0 - 2.0 * t)) * (d <= radius)).astype(np.float32)


def plume(seed=5, dims=(20, 16, 24), balls=7):
    """A small plume with every field populated (soot core, humid fringe, hot emitting base, age growing with height)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = dims
    density = np.zeros(dims, np.float32)
    for _ in range(balls):
        c = (rng.uniform(5, nx - 5), rng.uniform(3, ny - 4), rng.uniform(5, nz - 5))
        density += ball(dims, c, rng.uniform(3, 6), rng.uniform(0.2, 1.6))
    y = np.arange(ny, dtype=np.float32)[None, :, None]
    return {"density": density,
            "soot": (0.35 * density * (y < ny * 0.5)).astype(np.float32),
            "humidity": (0.8 * (density > 0.05) * (y / ny)).astype(np.float32),
            "temperature": (1.5 * density * (y < 6)).astype(np.float32),
            "emission_rate": (2.0 * density * (y < 4)).astype(np.float32),
            "particle_age": np.where(density > 1e-5, 20.0 * y / ny, -1.0).astype(np.float32)}


def _set(fields, size, settings=None, sun=SUN, voxel_size=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), frame_index=0, camera=None, view=None):
    return dict(fields=fields, size=size, settings=settings or {}, sun=sun, voxel_size=voxel_size, origin=origin, frame_index=frame_index,
                camera=camera, view=view, projection=view is not None)


def _camera(pos, target, fovy_deg, voxel_size=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """A camera given in voxel units, placed in the world of a grid with that voxel size and origin."""
    vs, og = np.array(voxel_size), np.array(origin)
    return dict(camera_pos=tuple(np.array(pos) * vs + og), target=tuple(np.array(target) * vs + og), up=up, fovy_deg=fovy_deg)


_SETS = None


def reference_sets():
    global _SETS
    if _SETS is not None:
        return _SETS
    dims = (20, 16, 24)
    nz, ny, nx = dims
    y = np.arange(ny, dtype=np.float32)[None, :, None]
    outside = _camera((12.3, 19.0, -21.0), (12.1, 7.2, 10.3), 42.0)
    sets = {}

    sets["plume"] = _set(plume(), (40, 30), camera=outside)

    f = plume(seed=11)
    d = f["density"]
    f.update(particle_age=np.where(d > 1e-5, 25.0 * y / (ny - 1), -1.0).astype(np.float32),  # 0 ... 25 s: both ramps, /9 and /17 into their clamps
             humidity=(1.3 * (d > 0.02) * (0.2 + y / ny)).astype(np.float32),                # over 1 (the clamp), milk into 0.38 where the body is dense
             temperature=(12.0 * d).astype(np.float32))                                      # the tint's heat into its clamp at 1
    sets["aged-humid"] = _set(f, (36, 28), camera=_camera((-13.0, 12.5, -11.0), (12.2, 8.1, 10.4), 40.0), sun=(-0.3, 0.6, -0.5))

    f = plume(seed=23)
    d = (f["density"] * 1.6).astype(np.float32)
    f.update(density=d, soot=(2.5 * d * (y > 3)).astype(np.float32), emission_rate=np.zeros(dims, np.float32))
    sets["sooty-dense"] = _set(f, (36, 28), dict(density_scale=2.5, extinction=4.0, soot_absorption=0.9, scattering=0.02, absorption=0.9,
                                                 thin_color=(0.2, 0.3, 0.4)), camera=outside)

    f = plume(seed=31)
    f.update(emission_rate=(6.0 * f["density"] * (y < 9)).astype(np.float32))
    sets["emitting"] = _set(f, (36, 28), dict(fire_glow=1.5, exposure=0.7), camera=outside, sun=(0.5, 0.7, 0.3))

    vs, og = (2.0, 1.5, 2.5), (-10.0, 3.0, 7.0)
    sets["non-cubic-offset"] = _set(plume(seed=5), (40, 30), dict(self_shadow=False, exposure=1.4, phase_g=-0.5), voxel_size=vs, origin=og,
                                    camera=_camera((12.3, 19.0, -21.0), (12.1, 7.2, 10.3), 42.0, vs, og))

    f = plume(seed=7, balls=10)
    sets["inside"] = _set(f, (36, 28), dict(step_size=0.4, shadow_step_size=1.1, shadow_steps=33, max_steps=900, jitter_strength=1.0), frame_index=77,
                          camera=_camera((12.3, 7.1, 9.6), (2.2, 3.1, 1.3), 80.0), sun=(-0.3, 0.5, 0.7))

    edge = np.zeros(dims, np.float32)
    edge[0, :, :] = 0.4
    edge[:, :, -1] = 0.7
    edge[:, 0, :] += 0.3
    edge[:, -1, :] += 0.2
    f = {"density": edge, "soot": (0.3 * edge).astype(np.float32), "particle_age": np.where(edge > 0, 5.0, -1.0).astype(np.float32)}
    sets["faces"] = _set(f, (36, 28), dict(shadow_steps=24, step_size=0.5, shadow_step_size=1.3), frame_index=3,
                         camera=_camera((12.3, 7.1, 9.6), (2.2, 3.1, 1.3), 80.0), sun=(0.0, 1.0, 0.0))

    f = plume(seed=13)
    f.update(soot=np.zeros(dims, np.float32))  # no soot and no absorption: the albedo into its clamp at 0.98
    sets["cut"] = _set(f, (36, 28), dict(max_steps=14, step_size=0.6, shadow_step_size=1.3, absorption=0.0, extinction=1.2), camera=outside)

    tdims = (10, 2, 12)  # ny = 2; the domain is 0.8 high, under the bounce term's floor of 1
    td = (ball(tdims, (5.0, 1.0, 4.0), 4.0, 1.4) + ball(tdims, (8.5, 0.5, 6.5), 3.0, 0.9)).astype(np.float32)
    f = {"density": td, "soot": (0.4 * td).astype(np.float32), "temperature": td.copy(), "particle_age": np.where(td > 0, 3.0, -1.0).astype(np.float32)}
    sets["thin"] = _set(f, (5, 3), voxel_size=(1.0, 0.4, 1.0), camera=dict(camera_pos=(6.2, 7.0, -5.1), target=(6.1, 0.4, 5.2), up=(0.0, 1.0, 0.0), fovy_deg=38.0))

    sets["projection"] = _set(plume(seed=17), (36, 28), view=(0.0, -1.0, 0.0))
    sets["projection-oblique"] = _set(plume(seed=19), (36, 28), dict(phase_g=0.6), view=(0.3, -0.8, 0.2), sun=(-0.5, 0.6, 0.2), frame_index=9)

    vs = (float(np.nextafter(np.float32(2.0), np.float32(0.0))), float(np.float32(1.0 / 3.0)), 1.0)  # the first: refused by div_known_divisor
    sets["awkward-voxel"] = _set(plume(seed=29), (36, 28), voxel_size=vs, origin=(1.5, -2.0, 0.25), camera=_camera((12.3, 19.0, -21.0), (12.1, 7.2, 10.3), 42.0, vs, (1.5, -2.0, 0.25)))
    # every edge under 1e-4: the default step is the floor, 0.75 * 1e-4 (1.5 of the smallest voxel), not 0.75 of a voxel
    vs, og = (5.0e-5, 6.0e-5, 7.0e-5), (1.0e-3, -2.0e-3, 5.0e-4)
    sets["tiny-voxel"] = _set(plume(seed=37), (36, 28), dict(extinction=2.6e4), voxel_size=vs, origin=og,
                              camera=_camera((12.3, 19.0, -21.0), (12.1, 7.2, 10.3), 42.0, vs, og))
    _SETS = sets
    return sets


def render_args(name_or_set):
    """(positional, keyword) arguments shared by the oracle's and the device's render calls of a set, without the settings."""
    s = reference_sets()[name_or_set] if isinstance(name_or_set, str) else name_or_set
    w, h = s["size"]
    if s["projection"]:
        return (w, h, s["view"], s["sun"]), {}
    return (w, h, s["camera"]["camera_pos"], s["camera"]["target"]), dict(up=s["camera"]["up"], fovy_deg=s["camera"]["fovy_deg"], sun_direction=s["sun"])


# ---- the fuzz scenes (tools/gpu_fuzz_smoke.py, tests/test_smoke.py) -----------------------------------------------------------
AWKWARD = [1.0, 0.5, 2.0, 1.0 / 3.0, 0.3, 0.7, 1.1, 7e-3, 0.015, 123.456, float(np.nextafter(np.float32(2.0), np.float32(0.0))), 3.0]


def case(seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = (int(rng.integers(2, 40)) for _ in range(3))
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    density = np.zeros((nz, ny, nx), np.float32)
    kind = int(rng.integers(0, 6))
    for _ in range(int(rng.integers(0, 5)) if kind else 0):  # kind 0: no smoke at all
        c = rng.uniform(-1, [nx, ny, nz]) + 0.5
        r = rng.uniform(0.6, 0.5 * max(nx, ny, nz))
        d = np.sqrt((x + 0.5 - c[0]) ** 2 + (y + 0.5 - c[1]) ** 2 + (z + 0.5 - c[2]) ** 2)
        density += (rng.uniform(0.05, 3.0) * np.clip(1.0 - d / r, 0.0, 1.0)).astype(np.float32)
    if kind == 1:  # a face of the grid
        density[:, :, 0 if rng.random() < 0.5 else -1] += np.float32(rng.uniform(0.1, 1.0))
    if kind == 2:  # lone voxels
        density[:] = 0
        for _ in range(3):
            density[int(rng.integers(nz)), int(rng.integers(ny)), int(rng.integers(nx))] = np.float32(rng.uniform(0.5, 4.0))
    fields = {"density": density, "soot": (rng.uniform(0, 0.6) * density * (rng.random(density.shape) < 0.7)).astype(np.float32),
              "temperature": (rng.uniform(0, 2.0) * density).astype(np.float32), "humidity": (rng.random(density.shape) * (density > 0.02)).astype(np.float32),
              "emission_rate": (rng.uniform(0, 2.0) * density * (y < ny * 0.3)).astype(np.float32),
              "particle_age": np.where(density > 1e-5, rng.uniform(0, 25.0) * y / max(1, ny), -1.0).astype(np.float32)}
    vs = tuple(float(np.float32(AWKWARD[int(rng.integers(len(AWKWARD)))] * (1.0 if rng.random() < 0.7 else rng.uniform(0.5, 2.0)))) for _ in range(3))
    og = tuple(float(v) for v in (rng.uniform(-50, 50, 3) if rng.random() < 0.7 else rng.uniform(-1, 1, 3) * 4000.0 * max(vs)))
    ext = np.array([nx, ny, nz]) * np.array(vs)
    centre = np.array(og) + 0.5 * ext
    if rng.random() < 0.3:  # camera inside the volume
        pos = np.array(og) + rng.uniform(0.05, 0.95, 3) * ext
    else:
        direction = rng.normal(size=3)
        pos = centre + direction / np.linalg.norm(direction) * rng.uniform(0.7, 3.0) * np.linalg.norm(ext)
    target = centre + rng.uniform(-0.3, 0.3, 3) * ext
    if rng.random() < 0.15:  # an axis-parallel central ray
        axis = int(rng.integers(3))
        pos = centre.copy()
        pos[axis] -= rng.uniform(0.8, 2.0) * ext[axis]
        target = centre.copy()
    sun = rng.normal(size=3)
    if rng.random() < 0.2:
        sun = np.eye(3)[int(rng.integers(3))] * (1 if rng.random() < 0.5 else -1)
    view = rng.normal(size=3)
    if rng.random() < 0.3:
        view = np.array([0.0, -1.0, 0.0])
    up = (0.0, 1.0, 0.0) if abs((target - pos)[1]) < 0.98 * np.linalg.norm(target - pos) else (1.0, 0.0, 0.0)
    st = dict(step_size=float(rng.uniform(0.2, 1.5) * min(vs)) if rng.random() < 0.8 else 0.0,
              shadow_step_size=float(rng.uniform(0.3, 3.0) * min(vs)) if rng.random() < 0.8 else 0.0,
              shadow_steps=int(rng.integers(1, 40)), max_steps=int(rng.choice([3, 17, 64, 200, 700])), self_shadow=bool(rng.random() < 0.85),
              jitter_strength=float(rng.uniform(0, 1)), density_scale=float(rng.uniform(0.3, 3.0)), extinction=float(rng.uniform(0.2, 4.0)),
              phase_g=float(rng.uniform(-0.8, 0.8)), soot_absorption=float(rng.uniform(0, 1.0)), fire_glow=float(rng.uniform(0, 2.0)))
    w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
    return fields, vs, og, tuple(pos), tuple(target), up, float(rng.uniform(15, 100)), tuple(sun), tuple(view), st, w, h, int(rng.integers(0, 1000))
