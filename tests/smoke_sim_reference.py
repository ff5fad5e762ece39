"""An independent float64 NumPy statement of one step of the smoke transport solver (csrc/f3d_smoke_sim.h, f3d_smoke_sim.hip,
oracle/smoke_sim_oracle.c) -- TEST INFRASTRUCTURE ONLY.  Nothing here comes from oracle/, tests/emul or the kernel headers: no
per-voxel function, no launch, no buffer twin.  Every pass is one whole-array expression over fields shaped (nz, ny, nx[, 3]),
written from what the step is defined to do (the reference's SmokeVolume::step and its helpers, src/smoke/sim.rs:7-799,
sampling.rs:1-94): finite differences are shifted slices, the trilinear sample is one gather, the grid sums are np.sum.

Inputs (the state's float32 arrays, the float32 settings and emitters) are promoted; everything after that is float64, with
NumPy's sin / cos / exp.  So the project's polynomial sin / cos / exp, its float32 rounding and its rows-then-slabs-then-total
summation order are what a comparison measures.

A step is discontinuous in three places, and the statement reports them instead of guessing which side float32 lands on:

  * particle_age jumps where the density after the decay crosses `sparse_threshold` and where a voxel centre crosses an
    emitter's radius: voxels within BAND_DENSITY (relative to the step's largest density after the decay; relative to the
    radius) of either are masked for particle_age;
  * the MacCormack clamp takes its eight cells from floor() of the back-traced position: a voxel one of whose back-traced
    coordinates lies within BAND_CELL voxel of a lattice plane WITHOUT being on it is masked for the five advected scalars
    (and for particle_age, which follows the density).  On the plane exactly is not ambiguous: that happens where a velocity
    component is exactly 0 (the borders), and float32 and float64 then agree exactly;
  * the confinement force normalises the gradient of |curl| unless its squared length is under 1e-12: `step` ASSERTS that no
    voxel of the margin-2 interior has a squared length under CONFINE_MIN_LEN2 -- a condition on the inputs, not an exclusion.

`step` returns the new state and, per field, the boolean mask of the voxels left out; a set may leave out at most BAND_CAP of
its voxels per field, which the tests assert of the reference alone.

The gates are MEASURED on the oracle, not chosen (tests/test_smoke_sim_reference_host.py part b prints them):

    python -m pytest -m "not gpu" tests/test_smoke_sim_reference_host.py -k oracle -s | grep smoke-ref

MEASURED_ON_THE_ORACLE holds, per set and field, the largest |oracle - reference| outside the bands over the set's steps (each
from the oracle's own float32 state of the step before), as a multiple of eps32 * max|reference| of that field in that step.
The gate is four times that, rounded up to two digits; the device has to equal the oracle bit for bit anyway
(tests/test_smoke_sim.py), so the factor covers nothing but the float64 libm's and NumPy's summation differences between
machines.  Neither the host nor the GPU test derives a tolerance from the code it checks.

What the measurement says: every field of every set stays within a few tens of eps32 of its largest value, and the "bare plus
one" sets sit within a unit or two of "bare" -- no pass stands out.  The advected scalars carry the rounding of the trilinear
samples (2-9 units; 15 in the density of old smoke, whose decay and eddies go through more
polynomial exp and smoothstep ramps), the velocity that of its own advection and two projections (8-13), the pressure one rounding a Jacobi
sweep (up to 31 after 20 + 10 sweeps).  The two sets with a hundred voxels in x ("case-wide", "edge-tile-plus-one") reach
43 in the velocity and 26-28 in density and humidity: a float32 back-traced position at x ~ 90 is rounded to 4e-6 voxel
(against 1e-7 at x ~ 2) and the field's slope carries that into the sample, and the sub-grid eddies' phases grow with x the
same way.  That error grows with the coordinate, as float32 rounding does, and is largest in the last tenth of the row.
"""
from __future__ import annotations

import math

import numpy as np

f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)

SCALARS = ("density", "temperature", "fuel", "soot", "humidity")  # the advected fields, in the step's order
FIELDS = SCALARS + ("emission_rate", "particle_age", "velocity", "pressure")

BAND_CELL = 1e-4          # voxels: the MacCormack clamp's cell is not compared this close to a lattice plane
BAND_DENSITY = 1.3e-5     # four times the density's largest measured error (4 x 26 eps32 = 1.24e-5), rounded up
BAND_CAP = 0.01           # a set may leave out at most this share of its voxels, per field
CONFINE_MIN_LEN2 = 1e-8   # squared length of grad |curl| that every margin-2 interior voxel of a test input must exceed

STEP_DEFAULTS = dict(dt=1.0 / 30.0, density_decay=0.015, temperature_decay=0.08, velocity_damping=0.01, diffusion=0.0005, buoyancy=0.7,
                     vorticity=0.12, pressure_iterations=20, turbulence_strength=0.0, turbulence_seed=0, mac_cormack=False,
                     mass_conservation=True, terrain_collision=True, boundary_damping=0.0, wind=(0.0, 0.0, 0.0))
EMITTER_DEFAULTS = dict(center=(0.0, 0.0, 0.0), radius=1.0, density_rate=1.0, temperature_rate=1.0, fuel_rate=0.0, soot_rate=0.2,
                        humidity_rate=0.0, emission_rate=1.0, velocity=(0.0, 1.0, 0.0), start_time=0.0, end_time=float(np.finfo(f32).max))

# set -> field -> the oracle's largest error outside the bands, in eps32 * max|reference| (see the module's docstring)
MEASURED_ON_THE_ORACLE = {
    "aged": {"density": 15, "temperature": 3.5, "fuel": 7.9, "soot": 8.3, "humidity": 8.8, "emission_rate": 0.56, "particle_age": 0.32, "velocity": 8.1, "pressure": 6.3},
    "bare": {"density": 3, "temperature": 2.3, "fuel": 2.5, "soot": 3.2, "humidity": 5.4, "emission_rate": 0.56, "particle_age": 0, "velocity": 12, "pressure": 8.6},
    "bare+damping": {"density": 2.5, "temperature": 2.6, "fuel": 2.3, "soot": 2.4, "humidity": 6.1, "emission_rate": 0.56, "particle_age": 0, "velocity": 13, "pressure": 9.9},
    "bare+diffusion": {"density": 2.7, "temperature": 2.8, "fuel": 3, "soot": 3.3, "humidity": 5.6, "emission_rate": 0.56, "particle_age": 0, "velocity": 12, "pressure": 8.1},
    "bare+maccormack": {"density": 2.1, "temperature": 1.7, "fuel": 1.7, "soot": 1.4, "humidity": 5.2, "emission_rate": 0.56, "particle_age": 0, "velocity": 12, "pressure": 8.6},
    "bare+mass": {"density": 3.2, "temperature": 2.3, "fuel": 2.5, "soot": 3.2, "humidity": 5.4, "emission_rate": 0.56, "particle_age": 0, "velocity": 12, "pressure": 8.6},
    "bare+pressure30": {"density": 2.8, "temperature": 2.8, "fuel": 2.8, "soot": 2.7, "humidity": 6.7, "emission_rate": 0.56, "particle_age": 0, "velocity": 12, "pressure": 11},
    "bare+turbulence-calm": {"density": 4.2, "temperature": 2.6, "fuel": 2.8, "soot": 2.9, "humidity": 6.4, "emission_rate": 0.56, "particle_age": 0, "velocity": 9.2, "pressure": 6.9},
    "bare+turbulence-wind": {"density": 4.6, "temperature": 2.2, "fuel": 2.3, "soot": 2.3, "humidity": 6, "emission_rate": 0.56, "particle_age": 0, "velocity": 7.6, "pressure": 9.2},
    "bare+vorticity": {"density": 2.7, "temperature": 2.6, "fuel": 2.5, "soot": 2.6, "humidity": 6, "emission_rate": 0.56, "particle_age": 0, "velocity": 12, "pressure": 8.2},
    "bare+voxel": {"density": 2.6, "temperature": 2.8, "fuel": 3, "soot": 2.6, "humidity": 5.9, "emission_rate": 0.94, "particle_age": 0, "velocity": 10, "pressure": 8.6},
    "case-bare": {"density": 8.8, "temperature": 2.8, "fuel": 2.6, "soot": 2.4, "humidity": 3.3, "emission_rate": 0.56, "particle_age": 0, "velocity": 4.8, "pressure": 5.2},
    "case-defaults": {"density": 3.3, "temperature": 2.7, "fuel": 2.5, "soot": 3.3, "humidity": 7.8, "emission_rate": 0.56, "particle_age": 0, "velocity": 9.8, "pressure": 31},
    "case-maccormack": {"density": 4, "temperature": 2.4, "fuel": 2.1, "soot": 1.8, "humidity": 3.7, "emission_rate": 0.56, "particle_age": 0.13, "velocity": 12, "pressure": 10},
    "case-six_emitters": {"density": 4.6, "temperature": 3.2, "fuel": 0, "soot": 4.3, "humidity": 7.8, "emission_rate": 1.1, "particle_age": 0, "velocity": 11, "pressure": 16},
    "case-turbulent_wind": {"density": 3.8, "temperature": 3.2, "fuel": 3.1, "soot": 2.7, "humidity": 9.1, "emission_rate": 0.94, "particle_age": 0.063, "velocity": 12, "pressure": 7.6},
    "case-wide": {"density": 4.2, "temperature": 3.1, "fuel": 3.5, "soot": 3.1, "humidity": 23, "emission_rate": 0.56, "particle_age": 0.13, "velocity": 43, "pressure": 40},
    "edge-first-margin2": {"density": 1.9, "temperature": 1.2, "fuel": 0, "soot": 1.1, "humidity": 1.3, "emission_rate": 0.56, "particle_age": 0, "velocity": 1.9, "pressure": 2.8},
    "edge-one-interior": {"density": 2.5, "temperature": 0.89, "fuel": 0, "soot": 1.2, "humidity": 0.8, "emission_rate": 0.56, "particle_age": 0, "velocity": 1.3, "pressure": 5.6},
    "edge-tile-plus-one": {"density": 26, "temperature": 1.4, "fuel": 0, "soot": 1.3, "humidity": 28, "emission_rate": 0.56, "particle_age": 0, "velocity": 43, "pressure": 31},
}


def gate(name, field):
    """Four times the recorded error, rounded up to two digits."""
    v = 4.0 * MEASURED_ON_THE_ORACLE[name][field]
    if v <= 0.0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - 1)
    return math.ceil(v / q - 1e-9) * q


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _p(v):
    """A float32 input, promoted."""
    return f64(f32(v))


def settings(**kw):
    """The step's settings as the float32 values the solver receives, promoted."""
    unknown = set(kw) - set(STEP_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown settings {sorted(unknown)}")
    s = {**STEP_DEFAULTS, **kw}
    out = {k: _p(s[k]) for k in ("dt", "density_decay", "temperature_decay", "velocity_damping", "diffusion", "buoyancy", "vorticity",
                                 "turbulence_strength", "boundary_damping")}
    out.update(pressure_iterations=int(s["pressure_iterations"]), turbulence_seed=int(s["turbulence_seed"]), mac_cormack=bool(s["mac_cormack"]),
               mass_conservation=bool(s["mass_conservation"]), terrain_collision=bool(s["terrain_collision"]),
               wind=tuple(_p(w) for w in s["wind"]))
    return out


def emitter(**kw):
    e = {**EMITTER_DEFAULTS, **kw}
    out = {k: _p(e[k]) for k in e if k not in ("center", "velocity")}
    out.update(center=tuple(_p(c) for c in e["center"]), velocity=tuple(_p(c) for c in e["velocity"]))
    return out


def promote(source, dims=None, voxel_size=None, origin=None, sparse_threshold=None, time_seconds=None, frame_index=None):
    """A float64 state from float32 arrays: `source` is a mapping or an object with the nine fields (and, unless given, dims
    (nx, ny, nz), voxel_size, origin, sparse_threshold, time_seconds, frame_index)."""
    get = (lambda k: source[k]) if isinstance(source, dict) else (lambda k: getattr(source, k))
    st = {}
    for name in FIELDS:
        a = np.asarray(get(name))
        assert a.dtype == f32, (name, a.dtype)
        st[name] = a.astype(f64)
    nz, ny, nx = st["density"].shape
    assert dims is None or tuple(dims) == (nx, ny, nz)
    assert st["velocity"].shape == (nz, ny, nx, 3)
    st["voxel_size"] = tuple(_p(v) for v in (voxel_size if voxel_size is not None else get("voxel_size")))
    st["origin"] = tuple(_p(v) for v in (origin if origin is not None else get("origin")))
    st["sparse_threshold"] = _p(sparse_threshold if sparse_threshold is not None else get("sparse_threshold"))
    st["time_seconds"] = _p(time_seconds if time_seconds is not None else get("time_seconds"))
    st["frame_index"] = int(frame_index if frame_index is not None else get("frame_index"))
    return st


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def lattice(shape):
    """(z, y, x) float64 index arrays of a (nz, ny, nx) grid."""
    nz, ny, nx = shape[:3]
    return np.meshgrid(np.arange(nz, dtype=f64), np.arange(ny, dtype=f64), np.arange(nx, dtype=f64), indexing="ij")


def _block(a, m, dz=0, dy=0, dx=0):
    """The voxels at least `m` from every face, displaced by (dz, dy, dx); empty when an axis has none."""
    idx = []
    for n, d in zip(a.shape[:3], (dz, dy, dx)):
        lo = m + d
        idx.append(slice(lo, max(n - m + d, lo)))
    return a[tuple(idx)]


def _central(a, m, axis):
    """a(+1) - a(-1) along `axis` (0 = z, 1 = y, 2 = x) over the margin-m interior."""
    d = [0, 0, 0]
    d[axis] = 1
    up = _block(a, m, *d)
    d[axis] = -1
    return up - _block(a, m, *d)


def smoothstep(e0, e1, x):
    t = np.clip((x - e0) / np.maximum(e1 - e0, 1.0e-6), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def trilinear(field, px, py, pz):
    """`field` ((nz, ny, nx) or (nz, ny, nx, 3)) at grid coordinates (px, py, pz), clamped to the grid."""
    nz, ny, nx = field.shape[:3]

    def cell(p, n):
        p = np.clip(np.asarray(p, f64), 0.0, n - 1.0)
        lo = np.floor(p).astype(np.intp)
        return lo, np.minimum(lo + 1, n - 1), p - lo

    (x0, x1, tx), (y0, y1, ty), (z0, z1, tz) = cell(px, nx), cell(py, ny), cell(pz, nz)
    if field.ndim == 4:
        tx, ty, tz = tx[..., None], ty[..., None], tz[..., None]
    mix = lambda a, b, t: a + (b - a) * t  # noqa: E731
    near = mix(mix(field[z0, y0, x0], field[z0, y0, x1], tx), mix(field[z0, y1, x0], field[z0, y1, x1], tx), ty)
    far = mix(mix(field[z1, y0, x0], field[z1, y0, x1], tx), mix(field[z1, y1, x0], field[z1, y1, x1], tx), ty)
    return mix(near, far, tz)


def departure(velocity, voxel_size, dt, sign=-1.0, start=None):
    """Where a voxel's content comes from (sign -1) or goes to (+1) in `dt`: (px, py, pz) in voxels.  `start`: positions to
    trace from instead of the voxel centres."""
    z, y, x = lattice(velocity.shape) if start is None else (start[2], start[1], start[0])
    v = trilinear(velocity, x, y, z)
    return (x + sign * v[..., 0] * dt / voxel_size[0], y + sign * v[..., 1] * dt / voxel_size[1], z + sign * v[..., 2] * dt / voxel_size[2])


# ---- the passes ------------------------------------------------------------------------------------------------------------
def emitter_distance(shape, voxel_size, origin, e):
    z, y, x = lattice(shape)
    return np.sqrt((origin[0] + (x + 0.5) * voxel_size[0] - e["center"][0]) ** 2 + (origin[1] + (y + 0.5) * voxel_size[1] - e["center"][1]) ** 2 +
                   (origin[2] + (z + 0.5) * voxel_size[2] - e["center"][2]) ** 2)


def emit(st, e, dt):
    """One emitter's smooth ball added to the fields of `st` (in place on the float64 copies `step` made)."""
    radius = max(e["radius"], 1.0e-6)
    d = emitter_distance(st["density"].shape, st["voxel_size"], st["origin"], e)
    inside = d <= radius
    falloff = np.where(inside, 1.0 - smoothstep(0.0, radius, d), 0.0)
    amount = dt * falloff
    for name in SCALARS:
        st[name] = np.where(inside, np.maximum(st[name] + e[name + "_rate"] * amount, 0.0), st[name])
    st["emission_rate"] = st["emission_rate"] + e["emission_rate"] * falloff
    st["particle_age"] = np.where(inside, 0.0, st["particle_age"])
    st["velocity"] = st["velocity"] + amount[..., None] * np.asarray(e["velocity"], f64)
    return np.abs(d - radius) < BAND_DENSITY * radius


def forces(velocity, temperature, s, time_seconds):
    """Wind, buoyancy, damping and the turbulence lanes."""
    dt, wind = s["dt"], s["wind"]
    v = velocity + np.stack([np.full_like(temperature, wind[0]), wind[1] + temperature * s["buoyancy"], np.full_like(temperature, wind[2])], -1) * dt
    if s["velocity_damping"] > 0.0:
        v = v * np.exp(-s["velocity_damping"] * dt)
    if s["turbulence_strength"] > 0.0:
        nz, ny, nx = temperature.shape
        z, y, x = lattice(temperature.shape)
        xf, yf, zf = x / max(nx - 1, 1), y / max(ny - 1, 1), z / max(nz - 1, 1)
        seed, t, amp = s["turbulence_seed"] * 0.000137, time_seconds, s["turbulence_strength"] * dt
        gain = np.clip(0.45 + 0.75 * yf, 0.35, 1.20)
        lane_a = np.sin(xf * 9.6 + zf * 4.2 + yf * 1.6 + t * 0.52 + seed)
        lane_b = np.cos(zf * 7.4 - xf * 5.1 + yf * 2.7 - t * 0.37 + seed * 1.7)
        roll = np.sin((xf + zf) * 3.9 - yf * 5.2 + t * 0.29 + seed * 0.6)
        push = np.stack([(0.62 * lane_a + 0.28 * roll) * amp * gain, (0.08 * lane_b - 0.05 * roll) * amp, (-0.56 * lane_b + 0.26 * lane_a) * amp * gain], -1)
        w = math.hypot(wind[0], wind[2])
        if w > 1.0e-6:
            wx, wz = wind[0] / w, wind[2] / w
            cx, cz = -wz, wx  # the horizontal direction across the wind
            along, across = x * wx + z * wz, x * cx + z * cz
            phase = along * 0.34 + across * 0.72 + t * 0.34 + seed * 11.0
            lane = np.sin(phase) + 0.45 * np.sin(phase * 0.53 + z * 0.29)
            speed = 0.5 + 0.5 * np.cos(phase * 0.41 + x * 0.18)
            shear = (yf - 0.42) * amp * 1.35
            push[..., 0] += cx * lane * amp * 0.82 * gain + wx * speed * amp * 0.30 * gain + cx * shear
            push[..., 2] += cz * lane * amp * 0.82 * gain + wz * speed * amp * 0.30 * gain + cz * shear
        v = v + push
    return v


def advect_velocity(velocity, voxel_size, dt):
    """The velocity carried along itself (semi-Lagrangian)."""
    bx, by, bz = departure(velocity, voxel_size, dt)
    return trilinear(velocity, bx, by, bz)


def diffuse(field, rate, dt):
    """One implicit-looking relaxation of the interior from the field before it; the border stays."""
    if rate <= 0.0:
        return field
    a = rate * dt
    out = field.copy()
    ring = sum(_block(field, 1, *d) for d in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)))
    _block(out, 1)[...] = (_block(field, 1) + a * ring) / (1.0 + 6.0 * a)
    return out


def curl(velocity, voxel_size):
    """(nz, ny, nx, 3): the curl by central differences in the interior, 0 on the border."""
    u, v, w = velocity[..., 0], velocity[..., 1], velocity[..., 2]
    hx, hy, hz = (2.0 * h for h in voxel_size)
    out = np.zeros_like(velocity)
    _block(out, 1)[..., 0] = _central(w, 1, 1) / hy - _central(v, 1, 0) / hz
    _block(out, 1)[..., 1] = _central(u, 1, 0) / hz - _central(w, 1, 2) / hx
    _block(out, 1)[..., 2] = _central(v, 1, 2) / hx - _central(u, 1, 1) / hy
    return out


def confine(velocity, voxel_size, strength, dt):
    """Vorticity confinement: N x curl * strength * dt over the margin-2 interior, N the unit gradient of |curl| (raw
    differences: no voxel size).  Returns the velocity and the squared gradient lengths of the margin-2 interior."""
    c = curl(velocity, voxel_size)
    mag = np.sqrt((c * c).sum(-1))
    g = np.stack([_central(mag, 2, 2), _central(mag, 2, 1), _central(mag, 2, 0)], -1)
    len2 = (g * g).sum(-1)
    with np.errstate(all="ignore"):
        n = np.where((len2 > 1.0e-12)[..., None], g / np.sqrt(len2)[..., None], 0.0)
    out = velocity.copy()
    _block(out, 2)[...] += np.cross(n, _block(c, 2)) * strength * dt
    return out, len2


def divergence(velocity, voxel_size):
    out = np.zeros(velocity.shape[:3])
    _block(out, 1)[...] = (_central(velocity[..., 0], 1, 2) / (2.0 * voxel_size[0]) + _central(velocity[..., 1], 1, 1) / (2.0 * voxel_size[1]) +
                           _central(velocity[..., 2], 1, 0) / (2.0 * voxel_size[2]))
    return out


def jacobi_sweep(pressure, div):
    """One sweep: the mean of the six neighbours less a sixth of the divergence in the interior, 0 on the border."""
    out = np.zeros_like(pressure)
    ring = sum(_block(pressure, 1, *d) for d in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)))
    _block(out, 1)[...] = (ring - _block(div, 1)) / 6.0
    return out


def subtract_gradient(velocity, pressure, voxel_size):
    out = velocity.copy()
    for c, axis in ((0, 2), (1, 1), (2, 0)):
        _block(out, 1)[..., c] -= _central(pressure, 1, axis) / (2.0 * voxel_size[c])
    return out


def project(velocity, voxel_size, iterations):
    """The pressure projection: `iterations` Jacobi sweeps from zero, then the gradient subtracted.  (velocity, pressure)."""
    div = divergence(velocity, voxel_size)
    p = np.zeros_like(div)
    for _ in range(int(iterations)):
        p = jacobi_sweep(p, div)
    return subtract_gradient(velocity, p, voxel_size), p


def boundaries(density, temperature, velocity, s):
    """Walls: the normal velocity component vanishes on every face; the x and z faces (and, weaker, the voxels next to them)
    swallow density and temperature, the y faces do not; the ground (y = 0) damps them with terrain collision."""
    nz, ny, nx = density.shape
    z, y, x = (a.astype(np.intp) for a in lattice(density.shape))
    vel = velocity.copy()
    vel[..., 0][(x == 0) | (x == nx - 1)] = 0.0
    vel[..., 1][(y == 0) | (y == ny - 1)] = 0.0
    vel[..., 2][(z == 0) | (z == nz - 1)] = 0.0

    def wall(i, n, face, beside):
        on = (i == 0) | (i == n - 1)
        return np.where(on, face, np.where((i == 1) | (i == n - 2), beside, 1.0))

    dens = density * wall(x, nx, 0.58, 0.78) * wall(z, nz, 0.58, 0.78)
    temp = temperature * wall(x, nx, 0.70, 0.86) * wall(z, nz, 0.70, 0.86)
    if s["terrain_collision"]:
        keep = np.where(y == 0, 1.0 - s["boundary_damping"], 1.0)
        dens, temp = dens * keep, temp * keep
    return dens, temp, vel


_EDDIES = ((5.5, 5.4, 1.0, 1.85), (11.5, 7.6, -1.0, 1.58), (19.0, 10.2, 1.0, 1.30), (28.0, 13.0, -1.0, 1.05))  # distance, radius, side, strength


def lane_shear(velocity, density, s, sparse_threshold, frame_index):
    """Cross-wind lanes, slabs and four eddies downwind of the smoke's centroid, acting where there is smoke."""
    w = math.hypot(s["wind"][0], s["wind"][2])
    if s["turbulence_strength"] <= 0.0 or w <= 1.0e-6:
        return velocity
    nz, ny, nx = density.shape
    z, y, x = lattice(density.shape)
    wx, wz = s["wind"][0] / w, s["wind"][2] / w
    cx, cz = -wz, wx
    amp, seed, fi = s["turbulence_strength"] * s["dt"], s["turbulence_seed"], f64(frame_index)
    mass = np.maximum(density, 0.0)
    total = np.sum(mass)
    centre_x, centre_z = np.sum(x * mass), np.sum(z * mass)
    if total > 1.0e-6:
        centre_x, centre_z = centre_x / total, centre_z / total
    active = smoothstep(sparse_threshold, max(sparse_threshold * 60.0, 0.012), density)
    along, across = x * wx + z * wz, x * cx + z * cz
    altitude = y / max(ny - 1, 1)
    lane_phase = along * 0.23 + across * 0.49 + fi * 0.105 + seed * 0.0027
    lane = np.sin(lane_phase) + 0.58 * np.sin(lane_phase * 0.41 + y * 0.74)
    sideways = (lane * 2.75 + (altitude - 0.44) * 0.95 * 1.45) * active * amp
    slab_phase = along * 0.17 - across * 0.31 + y * 1.12 + fi * 0.043 + seed * 0.0021
    slab = np.sin(slab_phase) + 0.42 * np.sin(slab_phase * 0.53 + along * 0.09)
    sideways = sideways + ((altitude - 0.50) * 2.55 + slab * 0.58) * active * amp * 1.90
    forward = np.sin(slab_phase * 0.39 + y * 0.67) * active * amp * 0.52
    dvx, dvz = cx * sideways + wx * forward, cz * sideways + wz * forward
    if total > 1.0e-6:
        for k, (distance, radius, side, strength) in enumerate(_EDDIES):
            phase = fi * (0.035 + k * 0.006) + seed * 0.0013
            ex = centre_x + wx * distance + cx * side * radius * (0.40 + 0.20 * np.sin(phase))
            ez = centre_z + wz * distance + cz * side * radius * (0.40 + 0.20 * np.cos(phase))
            rx, rz = x - ex, z - ez
            r2 = rx * rx + rz * rz
            spin = side * strength * amp * np.exp(-r2 / (2.0 * radius * radius)) * active * (0.55 + 0.75 * altitude) / np.sqrt(r2 + 1.0)
            dvx, dvz = dvx - rz * spin, dvz + rx * spin
    on = active > 0.0
    out = velocity.copy()
    out[..., 0] += np.where(on, dvx, 0.0)
    out[..., 2] += np.where(on, dvz, 0.0)
    return out


def advect_predict(field, back):
    """The semi-Lagrangian predictor: the field at the back-traced positions, never negative."""
    return np.maximum(trilinear(field, *back), 0.0)


def maccormack_band(back):
    """Voxels whose clamp cell is not certain: a back-traced coordinate within BAND_CELL of a lattice plane but not on it."""
    band = np.zeros(back[0].shape, bool)
    for p in back:
        r = np.abs(p - np.rint(p))
        band |= (r < BAND_CELL) & (r != 0.0)
    return band


def advect_correct(field, predicted, velocity, voxel_size, dt, back):
    """The MacCormack correction: half the round trip's error taken off the predictor, clamped to the eight cells around the
    back-traced position."""
    fwd = departure(velocity, voxel_size, dt, +1.0, start=back)
    candidate = predicted + 0.5 * (field - trilinear(predicted, *fwd))
    nz, ny, nx = field.shape
    lo3 = [np.clip(np.floor(p), 0, n - 1).astype(np.intp) for p, n in zip(back, (nx, ny, nz))]
    hi3 = [np.minimum(a + 1, n - 1) for a, n in zip(lo3, (nx, ny, nz))]
    corners = np.stack([field[zz, yy, xx] for zz in (lo3[2], hi3[2]) for yy in (lo3[1], hi3[1]) for xx in (lo3[0], hi3[0])])
    return np.maximum(np.clip(candidate, corners.min(0), corners.max(0)), 0.0)


def advect_scalar(field, velocity, voxel_size, dt, mac_cormack):
    back = departure(velocity, voxel_size, dt)
    predicted = advect_predict(field, back)
    return advect_correct(field, predicted, velocity, voxel_size, dt, back) if mac_cormack else predicted


def scale_to_mass(density, target):
    """The density rescaled so that its sum is `target` (the sum before the advection)."""
    mass = np.sum(density)
    return density * (target / mass) if target > 0.0 and mass > 1.0e-12 else density


def subgrid_eddies(density, humidity, particle_age, s, sparse_threshold, frame_index):
    """Sub-grid structure: voids, ridges, entrained clear air and channels modulate density and humidity where there is smoke."""
    if s["turbulence_strength"] <= 0.0:
        return density, humidity
    z, y, x = lattice(density.shape)
    w = max(math.hypot(s["wind"][0], s["wind"][2]), 1.0e-6)
    wx, wz = s["wind"][0] / w, s["wind"][2] / w
    cx, cz = -wz, wx
    seed, fi = s["turbulence_seed"], f64(frame_index)
    t = fi * 0.046
    active = smoothstep(sparse_threshold, max(sparse_threshold * 90.0, 0.018), density)
    wobble = np.sin(x * 0.043 + z * 0.071 + t + seed * 0.0019)
    phase = x * 0.18 + z * 0.27 + y * 0.72 + wobble * 1.7 + t + seed * 0.0019
    ribbons = 0.5 + 0.5 * np.sin(phase)
    sheets = 0.5 + 0.5 * np.sin(phase * 0.47 - z * 0.16 + y * 0.51)
    voids = smoothstep(0.45, 0.84, 1.0 - ribbons) * smoothstep(0.34, 0.76, 1.0 - sheets) * active
    ridges = smoothstep(0.62, 0.94, ribbons) * smoothstep(0.48, 0.90, sheets) * active
    age = smoothstep(2.0, 28.0, np.maximum(particle_age, 0.0))
    along, across = x * wx + z * wz, x * cx + z * cz
    channel_phase = (along * 0.115 + across * 0.52 + (0.5 + 0.5 * wobble) * 5.4 + np.sin(y * 0.62 + along * 0.035) * 0.85 + fi * 0.033 + seed * 0.0023)
    wave = 0.5 + 0.5 * np.sin(channel_phase) + 0.28 * np.sin(channel_phase * 0.47 - across * 0.19 + y * 0.34)
    slots = smoothstep(0.50, 0.94, 1.0 - (0.62 * ribbons + 0.38 * sheets))
    core = 1.0 - 0.56 * smoothstep(0.72, 1.75, density)
    clear_air = np.clip(smoothstep(0.58, 1.06, wave) * (0.54 + 0.46 * slots) * (0.28 + 0.72 * age) * active * core, 0.0, 1.0)
    channel = np.clip(smoothstep(0.42, 0.86, 1.0 - wave) * (0.55 + 0.45 * slots) * active * (0.42 + 0.58 * age) * core, 0.0, 1.0)
    thin_air, thin_channel = (0.024 + 0.055 * age) * clear_air, (0.045 + 0.070 * age) * channel
    gain = (1.0 - (0.62 + 0.32 * age) * voids + (0.075 - 0.045 * age) * ridges) * (1.0 - thin_air) * (1.0 - thin_channel)
    on = active > 0.0
    dens = np.where(on, np.clip(density * gain, 0.0, 8.0), density)
    hum = np.where(on, np.maximum(humidity * (1.0 - (0.15 + 0.10 * age) * voids - thin_air - thin_channel), 0.0), humidity)
    return dens, hum


def decay_and_age(st, s):
    """Exponential decay (faster for old smoke), then the age: restarted at 0 where smoke appears, advanced where it stays, -1
    in clear air.  Returns the band around the threshold."""
    dt = s["dt"]
    old = smoothstep(7.0, 36.0, np.maximum(st["particle_age"], 0.0))
    thinning = np.exp(-s["density_decay"] * dt * (1.0 + 3.0 * old))
    st["density"] = st["density"] * thinning
    st["fuel"] = st["fuel"] * thinning
    st["soot"] = st["soot"] * np.exp(-s["density_decay"] * dt * (0.42 + 1.15 * old))
    st["temperature"] = st["temperature"] * np.exp(-s["temperature_decay"] * dt)
    smoke = st["density"] > st["sparse_threshold"]
    st["particle_age"] = np.where(smoke, np.where(st["particle_age"] < 0.0, 0.0, st["particle_age"] + dt), -1.0)
    top = float(np.abs(st["density"]).max()) if st["density"].size else 0.0
    return np.abs(st["density"] - st["sparse_threshold"]) < BAND_DENSITY * top


def step(state, s, emitters=()):
    """One step of `state` (promote()) under `s` (settings()) and `emitters` (emitter() each).  Returns (the new state, a dict
    field -> bool (nz, ny, nx) mask of the voxels whose value the statement does not commit to)."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    dt, vs, thr = s["dt"], st["voxel_size"], st["sparse_threshold"]
    shape = st["density"].shape
    age_band = np.zeros(shape, bool)
    st["emission_rate"] = np.zeros(shape)
    for e in emitters:
        if e["start_time"] <= st["time_seconds"] <= e["end_time"]:
            age_band |= emit(st, e, dt)
    v = forces(st["velocity"], st["temperature"], s, st["time_seconds"])
    v = advect_velocity(v, vs, dt)
    v = diffuse(v, s["diffusion"], dt)
    if s["vorticity"] > 0.0:
        v, len2 = confine(v, vs, s["vorticity"], dt)
        assert len2.size == 0 or float(len2.min()) >= CONFINE_MIN_LEN2, f"input too close to the confinement's switch: {float(len2.min()):.3g}"
    v, _ = project(v, vs, max(s["pressure_iterations"], 1))
    st["density"], st["temperature"], v = boundaries(st["density"], st["temperature"], v, s)
    v = lane_shear(v, st["density"], s, thr, st["frame_index"])
    back = departure(v, vs, dt)
    cell_band = maccormack_band(back) if s["mac_cormack"] else np.zeros(shape, bool)
    mass_before = np.sum(st["density"])
    for name in SCALARS:
        st[name] = advect_scalar(st[name], v, vs, dt, s["mac_cormack"])
        if name == "density" and s["mass_conservation"]:
            st[name] = scale_to_mass(st[name], mass_before)
    st["density"], st["humidity"] = subgrid_eddies(st["density"], st["humidity"], st["particle_age"], s, thr, st["frame_index"])
    for name in SCALARS:
        st[name] = diffuse(st[name], s["diffusion"], dt)
    age_band |= decay_and_age(st, s)
    v, st["pressure"] = project(v, vs, max(s["pressure_iterations"] // 2, 1))
    st["density"], st["temperature"], st["velocity"] = boundaries(st["density"], st["temperature"], v, s)
    st["time_seconds"] = st["time_seconds"] + dt
    st["frame_index"] = st["frame_index"] + 1
    masks = {name: cell_band for name in SCALARS}
    masks["particle_age"] = age_band | cell_band
    for name in ("emission_rate", "velocity", "pressure"):
        masks[name] = np.zeros(shape, bool)
    return st, masks


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def residuals(got, want, masks):
    """field -> (largest |got - want| outside the field's band in eps32 * max|want|, share of the voxels left out).  A field
    that is identically 0 in the reference has to be 0: any difference is reported as inf."""
    out = {}
    for name in FIELDS:
        g, w, m = np.asarray(got[name], f64), want[name], masks[name]
        keep = ~m if w.ndim == 3 else np.broadcast_to(~m[..., None], w.shape)
        err = float(np.abs(g - w)[keep].max()) if keep.any() else 0.0
        unit = EPS32 * float(np.abs(w).max()) if w.size else 0.0
        out[name] = ((err / unit) if unit > 0.0 else (0.0 if err == 0.0 else math.inf), float(m.mean()) if m.size else 0.0)
    return out
