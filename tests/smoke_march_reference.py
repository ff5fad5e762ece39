"""An independent float64 NumPy statement of the smoke ray-marcher's two renders, perspective and projection
(csrc/f3d_smoke.hip, oracle/smoke_oracle.c) -- TEST INFRASTRUCTURE ONLY.  Nothing here comes from oracle/, tests/emul or the
kernel: it is written from what the render is defined to do (the reference's raymarch_rgba, raymarch_projection_rgba,
march_ray_rgba, sun_transmittance, smoke_color, ray_box_intersection, src/smoke/render.rs:7-400; grid_coord_from_world,
types.rs:387-405; sample_scalar and hash01, sampling.rs:1-34, :96-103), and it is a restatement in another form, not a
transliteration: one array per quantity over all pixels of the image, a loop over the step index only, the self-shadow
marches of a step as one (pixels, shadow steps) array whose optical depth is a cumulative sum, the trilinear sample as one
gather of eight weighted corners.  There is no per-pixel function, no tile, no occupancy map, no smoke box, no deferred list
and no polynomial exp.

Inputs (the float32 fields, settings, camera, sun) are promoted once; everything after that is float64 with NumPy's exp, sqrt
and tan.  The jitter hash is integer arithmetic and is stated exactly in uint32.  So what a comparison measures is the
project's arithmetic: float32 rounding, the polynomial exp_det, d * sqrt(d) for powf(d, 1.5), the accumulated `t += step`
(here t_k = t_start + k * step) and the 24 bits that hash01 keeps of its 32-bit hash.

The shading's constants live in CONSTANTS, and `render` / `sun_transmittance` take a replacement table, so that a test can
perturb one at a time (tests/test_smoke_march_reference_host.py part c).  The self-shadow march repeats the ray's age ramp and
concentration gate as literals of its own in the reference, so they are entries of their own here (`shadow_*`): a misreading
of one place must not hide behind the other.  STRUCTURE holds three choices a port could get wrong without changing a number.

A ray is discontinuous in a few places.  `render` reports them as per-pixel boolean masks with a reason instead of guessing
which side float32 lands on (`masked` is their union):

  * "silhouette": the chord far - max(near, 0) through the domain box is within BAND_T * scale of empty, where scale is the
    larger of the box's diagonal and its largest absolute coordinate (the magnitude of the numbers whose float32 rounding moves
    near and far).  BAND_T = 1e-5 is 84 eps32: a slab distance is a difference, a reciprocal and a product (1.5 eps32 of a
    number up to ~3 scale for the case cameras) and t adds up to ~60 roundings of half an ulp of t, 30 eps32 at worst, ~4 rms.
  * "step-count": a step parameter t_k within the same band of t1 (either side), counted only if the step would contribute
    (interpolated density there > 0) and the ray is still running.  "shadow-step": the same for a self-shadow step
    t_i = t0 + (i + 0.5) * shadow_step against its t1 (`t > t1` ends that march), for any shading point of the pixel, counted
    only before the march's own `od > 8` end.
  * "opacity-cut": the running transmittance within BAND_CUT = 1e-4 (relative) of 0.01 after any step; one step more or less
    moves alpha by up to 0.01 = 2.5 codes.  The transmittance is a product of up to ~100 factors exp(-x), x < ~5, each good to
    ~(2 + x) eps32: 1e-4 is 840 eps32, above the worst case of their sum.
  * "unpremultiply": alpha within BAND_ALPHA = 2e-6 (absolute) of 1e-5, where rgb / alpha switches to rgb; alpha = 1 - T has
    an absolute float32 error of a few eps32.
  * faint pixels (`faint`, not part of `masked`): alpha below ALPHA_FLOOR = 1 / 255, one code.  1 - T has lost its digits
    there in float32 (T carries ~eps32 * sqrt(steps), so alpha carries that over alpha: 1e-4 and worse under the floor), and
    rgb / alpha inherits it.  RGB is compared there only premultiplied (colour * alpha), never as straight colour.

Not masked, because continuous to well under a code: `density > 1e-5` (a step at the threshold has sigma_t * step < 1e-4 for
the case settings, so it moves alpha and the premultiplied colour by < 1e-4 of a light term, 0.03 code; in float terms the
jump is smaller than the band of the faint floor and the sets' gates measure it); `sigma_t > 1e-6` (both branches of the
segment weight are `step` to within sigma_t * step / 2 < 1e-6 relative); `od > 8` (the march ends with exp(-8) = 3.4e-4 of a
light term left, and the step that crosses 8 is taken on both sides of the comparison).

Zero directions: ray_box_intersection yields NaN where a ray is parallel to a slab and starts exactly on one of its planes
(0 * inf); np.fmin / np.fmax drop the NaN as f32::min / max do, the case has measure zero, and the case cameras and suns
avoid exact zeros except `faces` (a sun along +y) and `projection` (the map's vertical view), whose rays start strictly
between the x and z faces.

`render` returns, per pixel, the unquantised straight RGB after the tone map, alpha, the transmittance, the step count, the
masks and `faint`.  A set may leave out at most MASK_CAP = 2 % of its pixels with reference alpha above the floor, which the
host test asserts of the reference alone.

The gates are MEASURED on the oracle's float march (smoke_oracle.hook_march), not chosen
(tests/test_smoke_march_reference_host.py part b prints them):

    python -m pytest -m "not gpu" tests/test_smoke_march_reference_host.py -s | grep smoke-march-ref

MEASURED_ON_THE_ORACLE holds, per set and channel, the largest |oracle - reference| outside the masks as a multiple of
eps32 * max|reference| of that channel.  `gate` is four times that, rounded up to two digits; the device has to equal the
oracle bit for bit anyway (tests/test_smoke.py), so the factor covers nothing but libm and NumPy differences between
machines.  The 8-bit gates (`code_gate`, `bias_gate`) are derived from the float gate, not measured anew:
|code - 255 v_ref| <= 0.5 + G with G = 255 * gate * eps32 * max|reference|, and |mean(code - 255 v_ref)| <= 4 * 0.5 / sqrt(N) + G
over the N unmasked pixels above the floor.  The rounding to a code is a near-uniform error of +-0.5, whose mean over N pixels
has a standard deviation of 0.29 / sqrt(N): the bias gate is seven of those, and it is what catches a small systematic error
-- a constant off by a part in a thousand moves every pixel the same way by a fraction of a code, invisible to the per-pixel
gate under the rounding, but not to the mean.

What the measurement says (in full above MEASURED_ON_THE_ORACLE): nothing but rounding.  Every channel of every set is within
110 eps32 of its largest value.  The colour's error is that of rgb / alpha in the faintest compared pixels (alpha 0.004 ... 0.008,
50 ... 110 eps32; 2 ... 4 where alpha > 0.2), alpha's and the transmittance's that of float32 sample positions at t ~ 30 ... 50 on
half-transparent rays seen from outside (10 ... 24; 1 ... 3 from inside the smoke).  The largest masked share is 0.4 % ("faces").
"""
from __future__ import annotations

import math

import numpy as np

f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)

BAND_T = 1e-5        # of the box's scale: silhouette, step count, self-shadow step count
BAND_CUT = 1e-4      # relative, of the opacity cut-off
BAND_ALPHA = 2e-6    # absolute, of the un-premultiply switch
ALPHA_FLOOR = 1.0 / 255.0
MASK_CAP = 0.02
CHANNELS = ("r", "g", "b", "alpha", "transmittance")

SETTINGS_DEFAULTS = dict(density_scale=1.0, extinction=2.6, scattering=0.85, absorption=0.45, phase_g=0.24, step_size=0.0, max_steps=256,
                         self_shadow=True, shadow_steps=20, shadow_step_size=0.0, jitter_strength=0.5, exposure=1.0,
                         thin_color=(0.50, 0.54, 0.58), dense_color=(0.93, 0.91, 0.82), soot_absorption=0.22, fire_glow=0.35)  # types.rs

# The literals of the shading, by the place they stand in (render.rs / types.rs / sampling.rs): every one but the 0 and 1 that end
# a clamp, the 1 of a complement or an increment (1 - x, 1 + x), the pi of the phase function and the integers of the jitter hash
# (which test_jitter_hash_against_hand_computed_seeds pins).
CONSTANTS = dict(
    # the image and the ray
    pixel_centre=0.5, plane_height=0.5, cell_centre=0.5, jitter_centre=0.5, step_fraction=0.75, shadow_step_ratio=2.0, min_step=1.0e-4,
    parallel=1.0e-12, half_fov=0.5, px_span=2.0, px_centre=1.0, py_centre=1.0, py_span=2.0,
    # render_smoothstep (one function for the ray and the self-shadow march)
    smooth_floor=1.0e-6, smooth_cubic=3.0, smooth_slope=2.0,
    # the ray's density
    age_lo=1.6, age_hi=17.0, age_thin=0.58, gate_base=0.50, gate_gain=0.50, gate_lo=0.045, gate_hi=0.34, density_floor=1.0e-5,
    ray_soot=0.85, sigma_floor=1.0e-6, opacity_cut=0.01,
    # the self-shadow march's own copy
    shadow_centre=0.5, shadow_age_lo=1.6, shadow_age_hi=17.0, shadow_age_thin=0.58, shadow_gate_base=0.50, shadow_gate_gain=0.50,
    shadow_gate_lo=0.045, shadow_gate_hi=0.34, shadow_od_cut=8.0,
    # phase, albedo
    phase_floor=1.0e-4, phase_power=1.5, phase_cross=2.0, phase_norm=4.0, albedo_soot=0.55, albedo_eps=1.0e-5, albedo_lo=0.02, albedo_hi=0.98,
    # the lights
    sun_r=1.0, sun_g=0.96, sun_b=0.84, sun_gain=11.5,
    sky_r=0.52, sky_g=0.60, sky_b=0.72, sky_base=0.36, sky_shadow=0.26, sky_soot=0.32, sky_soot_lo=0.50,
    bounce_r=0.58, bounce_g=0.54, bounce_b=0.48, bounce_gain=0.070, bounce_min_height=1.0,
    powder_depth=2.2, powder_gain=0.055,
    fire_r=1.0, fire_g=0.30, fire_b=0.055, fire_fresh=17.0, fire_heat=0.10, fire_emission=1.18, fire_clamp=5.0,
    # smoke_color
    body_density=1.45, body_soot=1.35, aged_span=9.0, aged_r=0.36, aged_g=0.39, aged_b=0.43, aged_mix=0.42,
    milk_base=0.18, milk_body=0.42, milk_r=0.93, milk_g=0.92, milk_b=0.84, milk_clamp=0.38,
    tint_fresh=17.0, tint_heat=0.12, tint_r=0.95, tint_g=0.62, tint_b=0.28, tint_mix=0.07,
    # the tone map
    alpha_switch=1.0e-5, tone_knee=1.0,
)

# Choices a port can get wrong without misreading a number: the self-shadow march carries no `ray_soot` on its soot term, the
# bounce term measures p.y from world zero (not from the domain's floor), and both marches clamp t0 at 0.
STRUCTURE = dict(shadow_soot_factor=False, bounce_from_floor=False, clamp_t0=True)

# set -> channel -> the oracle's largest error outside the masks, in eps32 * max|reference| of the channel (module docstring).
# What it shows.  Nothing but rounding: every channel of every set is within ~110 eps32 (1.3e-5) of its largest value, a
# thirtieth of a code.  The colour's largest errors all sit in the faintest compared pixels, alpha 0.004 ... 0.008 just above
# the floor, where alpha = 1 - T has ~2 eps32 of absolute error and the division rgb / alpha turns that into 50 ... 110 eps32 of
# the colour; pixels with alpha over 0.2 stay within 2 ... 4 eps32 in every set.  Alpha and the transmittance are worst
# (10 ... 24) in half-transparent pixels seen from outside: a sample position origin + dir * t at t ~ 30 ... 50 is rounded to 2e-6
# of a voxel, and the density's slope carries that into every step's extinction.  "inside" (t < 15, steps of 0.4) stays within
# 1 ... 3 in all channels, "thin" and "faces" (few steps, little slope) within 20.  The projections and "awkward-voxel" carry
# the most colour error because their faint fringes are the longest rays (the pull-back by the box's diagonal; 85 steps).
MEASURED_ON_THE_ORACLE = {
    "plume": {"r": 53, "g": 65, "b": 72, "alpha": 24, "transmittance": 24},
    "aged-humid": {"r": 34, "g": 44, "b": 50, "alpha": 15, "transmittance": 14},
    "sooty-dense": {"r": 43, "g": 27, "b": 39, "alpha": 23, "transmittance": 23},
    "emitting": {"r": 36, "g": 38, "b": 66, "alpha": 19, "transmittance": 19},
    "non-cubic-offset": {"r": 27, "g": 35, "b": 42, "alpha": 11, "transmittance": 11},
    "inside": {"r": 2.1, "g": 3.1, "b": 3.3, "alpha": 1.2, "transmittance": 3.1},
    "faces": {"r": 19, "g": 18, "b": 15, "alpha": 8.9, "transmittance": 8.5},
    "cut": {"r": 53, "g": 49, "b": 49, "alpha": 14, "transmittance": 14},
    "thin": {"r": 15, "g": 16, "b": 17, "alpha": 4.4, "transmittance": 4.3},
    "projection": {"r": 72, "g": 67, "b": 56, "alpha": 7.2, "transmittance": 7.2},
    "projection-oblique": {"r": 75, "g": 97, "b": 110, "alpha": 9.9, "transmittance": 9.9},
    "awkward-voxel": {"r": 57, "g": 88, "b": 110, "alpha": 12, "transmittance": 12},
    "tiny-voxel": {"r": 57, "g": 60, "b": 65, "alpha": 15, "transmittance": 15},
}


def gate(name, channel):
    """Four times the recorded error, rounded up to two digits (eps32 * max|reference| of the channel)."""
    v = 4.0 * MEASURED_ON_THE_ORACLE[name][channel]
    if v <= 0.0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - 1)
    return math.ceil(v / q - 1e-9) * q


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _p(v):
    """A float32 input, promoted."""
    return np.asarray(v, f32).astype(f64)


def volume(fields, voxel_size=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), frame_index=0):
    """The six render fields shaped (nz, ny, nx), promoted (missing ones are zeros, the age -1 as SmokeVolume::new leaves it)."""
    density = _p(fields["density"])
    nz, ny, nx = density.shape
    vol = {"density": density, "dims": np.array([nx, ny, nz]), "voxel": _p(voxel_size), "origin": _p(origin), "frame_index": int(frame_index) & 0xFFFFFFFF}
    for name, fill in (("temperature", 0.0), ("soot", 0.0), ("humidity", 0.0), ("emission_rate", 0.0), ("particle_age", -1.0)):
        vol[name] = _p(fields[name]) if name in fields else np.full(density.shape, fill)
    vol["lo"] = vol["origin"]
    vol["hi"] = vol["origin"] + vol["dims"] * vol["voxel"]
    return vol


def settings(**kw):
    s = {**SETTINGS_DEFAULTS, **kw}
    out = {k: (_p(v) if k in ("thin_color", "dense_color") else v) for k, v in s.items()}
    for k in ("density_scale", "extinction", "scattering", "absorption", "phase_g", "step_size", "shadow_step_size", "jitter_strength", "exposure",
              "soot_absorption", "fire_glow"):
        out[k] = float(f32(s[k]))
    return out


def step_sizes(vol, st, K=CONSTANTS):
    step = st["step_size"] if st["step_size"] > 0.0 else max(float(vol["voxel"].min()), K["min_step"]) * K["step_fraction"]
    shadow = st["shadow_step_size"] if st["shadow_step_size"] > 0.0 else step * K["shadow_step_ratio"]
    return step, shadow


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


# ---- primitives ------------------------------------------------------------------------------------------------------------
def hash01(seed):
    """sampling.rs:96-103, exactly in uint32; the quotient by 2^32 (u32::MAX as f32) in float64, all 32 bits kept."""
    v = np.asarray(seed, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & m
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & m
    v = v ^ (v >> np.uint64(16))
    return v.astype(f64) / 4294967296.0


def jitter_seed(x, y, frame_index, projection):
    m = np.uint64(0xFFFFFFFF)
    s = (np.asarray(x, np.uint64) * np.uint64(73856093)) & m
    s = (s + ((np.asarray(y, np.uint64) * np.uint64(19349663)) & m) + np.uint64(frame_index)) & m
    return (s + np.uint64(0x9E3779B9)) & m if projection else s


def ray_box(origin, direction, lo, hi, K=CONSTANTS):
    """near, far and whether the ray meets the box (far >= max(near, 0)); origins (..., 3), one direction or one per origin."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.broadcast_to(direction, origin.shape)
        inv = np.where(np.abs(d) > K["parallel"], 1.0 / np.where(d == 0.0, 1.0, d), np.inf)
        a, b = (lo - origin) * inv, (hi - origin) * inv
        near = np.fmax.reduce(np.fmin(a, b), axis=-1)
        far = np.fmin.reduce(np.fmax(a, b), axis=-1)
    return near, far, far >= np.maximum(near, 0.0)


def _corners(vol, pos, K):
    """Flat indices (..., 8) and trilinear weights (..., 8) of the eight voxels around world positions (..., 3)."""
    g = (pos - vol["origin"]) / vol["voxel"] - K["cell_centre"]
    top = (vol["dims"] - 1).astype(f64)
    g = np.clip(g, 0.0, top)
    i0 = np.floor(g)
    f = g - i0
    i0 = i0.astype(np.int64)
    i1 = np.minimum(i0 + 1, vol["dims"] - 1)
    nx, ny = int(vol["dims"][0]), int(vol["dims"][1])
    idx, wgt = [], []
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                ix = (i1 if cx else i0)[..., 0]
                iy = (i1 if cy else i0)[..., 1]
                iz = (i1 if cz else i0)[..., 2]
                idx.append((iz * ny + iy) * nx + ix)
                wgt.append((f[..., 0] if cx else 1.0 - f[..., 0]) * (f[..., 1] if cy else 1.0 - f[..., 1]) * (f[..., 2] if cz else 1.0 - f[..., 2]))
    return np.stack(idx, -1), np.stack(wgt, -1)


def _gather(vol, name, corners):
    idx, wgt = corners
    return np.sum(vol[name].reshape(-1)[idx] * wgt, axis=-1)


def sample(vol, name, pos, K=CONSTANTS):
    """The field's trilinear value at world positions (..., 3) (grid_coord_from_world, then sample_scalar)."""
    return _gather(vol, name, _corners(vol, np.asarray(pos, f64), K))


def smoothstep(e0, e1, x, K=CONSTANTS):
    t = np.clip((x - e0) / max(e1 - e0, K["smooth_floor"]), 0.0, 1.0)
    return t * t * (K["smooth_cubic"] - K["smooth_slope"] * t)


def _mix(a, b, t):
    return a + (b - a) * t[..., None]


def smoke_color(density, soot, humidity, temperature, age, st, K=CONSTANTS):
    """render.rs:329-346 over arrays; returns (..., 3)."""
    body = np.clip(density * K["body_density"] + soot * K["body_soot"], 0.0, 1.0)
    color = _mix(st["thin_color"], st["dense_color"], body)
    color = _mix(color, np.array([K["aged_r"], K["aged_g"], K["aged_b"]]), np.clip(age / K["aged_span"], 0.0, 1.0) * K["aged_mix"])
    milk = np.clip(humidity, 0.0, 1.0) * (K["milk_base"] + K["milk_body"] * body)
    color = _mix(color, np.array([K["milk_r"], K["milk_g"], K["milk_b"]]), np.clip(milk, 0.0, K["milk_clamp"]))
    heat = np.clip(temperature * K["tint_heat"] * np.clip(1.0 - age / K["tint_fresh"], 0.0, 1.0), 0.0, 1.0)
    return _mix(color, np.array([K["tint_r"], K["tint_g"], K["tint_b"]]), heat * K["tint_mix"])


def phase(cos_theta, g, K=CONSTANTS):
    denom = np.maximum(1.0 + g * g - K["phase_cross"] * g * cos_theta, K["phase_floor"])
    return (1.0 - g * g) / (K["phase_norm"] * math.pi * denom ** K["phase_power"])


# ---- the self-shadow march ---------------------------------------------------------------------------------------------------
def _sun_march(vol, points, sun, step, steps, st, K, S, scale):
    """Transmittance towards the sun from points (n, 3), and per point whether a step of the march lies in the band of its t1."""
    start = points + sun * step
    near, far, hit = ray_box(start, sun, vol["lo"], vol["hi"], K)
    t0 = np.maximum(near, 0.0) if S["clamp_t0"] else near
    with np.errstate(invalid="ignore"):
        t = t0[:, None] + (np.arange(steps, dtype=f64) + K["shadow_centre"]) * step  # (n, steps)
        t = np.where(hit[:, None], t, 0.0)
        inside = hit[:, None] & (t <= far[:, None])
        close = hit[:, None] & (np.abs(t - far[:, None]) < BAND_T * scale)
    c = _corners(vol, points[:, None, :] + sun * (step + t)[..., None], K)
    density, soot = _gather(vol, "density", c), _gather(vol, "soot", c)
    age = np.maximum(_gather(vol, "particle_age", c), 0.0)
    soot_term = 1.0 + soot * st["soot_absorption"] * (K["ray_soot"] if S["shadow_soot_factor"] else 1.0)
    depth = (density * st["density_scale"] * (1.0 - K["shadow_age_thin"] * smoothstep(K["shadow_age_lo"], K["shadow_age_hi"], age, K))
             * (K["shadow_gate_base"] + K["shadow_gate_gain"] * smoothstep(K["shadow_gate_lo"], K["shadow_gate_hi"], density, K))
             * st["extinction"] * soot_term * step)
    run = np.cumsum(np.where(inside, depth, 0.0), axis=1)
    over = run > K["shadow_od_cut"]
    first = np.where(over.any(axis=1), np.argmax(over, axis=1), steps - 1)  # the step after which the march ends
    od = run[np.arange(len(points)), first]
    reached = np.arange(steps)[None, :] <= first[:, None]
    ambiguous = (close & reached & (depth > 0.0)).any(axis=1)
    return np.where(hit, np.clip(np.exp(-od), 0.0, 1.0), 1.0), ambiguous


def _scale(vol):
    return float(max(np.sqrt(np.sum((vol["hi"] - vol["lo"]) ** 2)), np.abs(vol["lo"]).max(), np.abs(vol["hi"]).max()))


def sun_transmittance(vol, points, sun_direction, step, steps, st, K=CONSTANTS, S=STRUCTURE):
    """render.rs:278-316 at points (n, 3): `step` and `steps` are the march's own, the sun direction is used as given."""
    points = np.atleast_2d(_p(points))
    return _sun_march(vol, points, _p(sun_direction), float(f32(step)), int(steps), st, K, S, _scale(vol))[0]


# ---- the two renders -------------------------------------------------------------------------------------------------------
def _rays(vol, width, height, st, K, projection, camera_pos, target, up, fovy_deg, view_direction):
    x, y = np.meshgrid(np.arange(width, dtype=f64), np.arange(height, dtype=f64))
    x, y = x.reshape(-1), y.reshape(-1)
    if projection:
        direction = _unit(_p(view_direction))
        fx, fz = (x + K["pixel_centre"]) / width, (y + K["pixel_centre"]) / height
        lo, hi = vol["lo"], vol["hi"]
        plane = np.stack([lo[0] + (hi[0] - lo[0]) * fx, np.full_like(fx, (lo[1] + hi[1]) * K["plane_height"]), lo[2] + (hi[2] - lo[2]) * fz], -1)
        # the pull-back: any distance that leaves the origin outside the box gives the same samples (t0 is the box's entry)
        back = max(float(np.sqrt(np.sum((hi - lo) ** 2))), 2.0 * step_sizes(vol, st, K)[0])
        return plane - direction * back, np.broadcast_to(direction, plane.shape)
    eye = _p(camera_pos)
    forward = _unit(_p(target) - eye)
    right = _unit(np.cross(forward, _unit(_p(up))))
    camera_up = _unit(np.cross(right, forward))
    tan_half = np.tan(np.deg2rad(float(f32(fovy_deg))) * K["half_fov"])
    px = ((x + K["pixel_centre"]) / width * K["px_span"] - K["px_centre"]) * (width / height) * tan_half
    py = (K["py_centre"] - (y + K["pixel_centre"]) / height * K["py_span"]) * tan_half
    direction = _unit(forward + right * px[:, None] + camera_up * py[:, None])
    return np.broadcast_to(eye, direction.shape), direction


def render(vol, width, height, st, sun_direction, projection=False, camera_pos=None, target=None, up=(0.0, 1.0, 0.0), fovy_deg=45.0,
           view_direction=(0.0, -1.0, 0.0), K=CONSTANTS, S=STRUCTURE):
    """raymarch_rgba (projection=False) or raymarch_projection_rgba of `vol` under settings `st` (from `settings`).  Returns a
    dict of (height, width[, 3]) arrays: rgb (straight, tone-mapped, unquantised), alpha, transmittance, steps, `reasons` (name ->
    boolean mask), `masked` (their union) and `faint` (alpha below ALPHA_FLOOR)."""
    n = width * height
    origin, direction = _rays(vol, width, height, st, K, projection, camera_pos, target, up, fovy_deg, view_direction)
    sun = _unit(_p(sun_direction))
    step, shadow_step = step_sizes(vol, st, K)
    scale = _scale(vol)
    band = BAND_T * scale
    near, far, hit = ray_box(origin, direction, vol["lo"], vol["hi"], K)
    with np.errstate(invalid="ignore"):
        reasons = {"silhouette": np.abs(far - np.maximum(near, 0.0)) < band}
    for name in ("step-count", "shadow-step", "opacity-cut"):
        reasons[name] = np.zeros(n, bool)
    t0 = np.maximum(near, 0.0) if S["clamp_t0"] else near
    yy, xx = np.divmod(np.arange(n), width)
    jitter = (hash01(jitter_seed(xx, yy, vol["frame_index"], projection)) - K["jitter_centre"]) * st["jitter_strength"] * step
    t_start = np.maximum(np.where(hit, t0, 0.0) + jitter, 0.0)
    far = np.where(hit, far, -np.inf)

    cos_theta = np.clip(np.sum(direction * sun, axis=-1), -1.0, 1.0)
    sun_radiance = np.array([K["sun_r"], K["sun_g"], K["sun_b"]]) * K["sun_gain"]
    sky_colour = np.array([K["sky_r"], K["sky_g"], K["sky_b"]])
    bounce_colour = np.array([K["bounce_r"], K["bounce_g"], K["bounce_b"]]) * K["bounce_gain"]
    fire_colour = np.array([K["fire_r"], K["fire_g"], K["fire_b"]])
    floor_y = float(vol["lo"][1]) if S["bounce_from_floor"] else 0.0
    height_scale = max(float(vol["hi"][1]), K["bounce_min_height"])

    trans, rgb, steps = np.ones(n), np.zeros((n, 3)), np.zeros(n, np.int64)
    k = 0
    while True:
        t = t_start + k * step
        running = hit & (steps < st["max_steps"]) & (trans > K["opacity_cut"])
        active = running & (t < far)
        close = running & (np.abs(t - far) < band)
        sel = np.nonzero(active | close)[0]
        if sel.size == 0:
            break
        p = origin[sel] + direction[sel] * t[sel, None]
        c = _corners(vol, p, K)
        raw = _gather(vol, "density", c)
        reasons["step-count"][sel] |= close[sel] & (raw > 0.0)
        age = np.maximum(_gather(vol, "particle_age", c), 0.0)
        density = np.maximum(raw * st["density_scale"] * (1.0 - K["age_thin"] * smoothstep(K["age_lo"], K["age_hi"], age, K))
                             * (K["gate_base"] + K["gate_gain"] * smoothstep(K["gate_lo"], K["gate_hi"], raw, K)), 0.0)
        lit = active[sel] & (density > K["density_floor"])
        steps[sel] += active[sel]
        k += 1
        if not lit.any():
            continue
        sel, p, c, raw, age, density = sel[lit], p[lit], (c[0][lit], c[1][lit]), raw[lit], age[lit], density[lit]
        soot, humidity = _gather(vol, "soot", c), _gather(vol, "humidity", c)
        temperature, emission = _gather(vol, "temperature", c), _gather(vol, "emission_rate", c)
        sigma_t = density * st["extinction"] * (1.0 + soot * st["soot_absorption"] * K["ray_soot"])
        seg_trans = np.clip(np.exp(-sigma_t * step), 0.0, 1.0)
        seg_weight = np.where(sigma_t > K["sigma_floor"], (1.0 - seg_trans) / np.maximum(sigma_t, 1e-300), step)
        if st["self_shadow"]:
            light, ambiguous = _sun_march(vol, p, sun, shadow_step, int(st["shadow_steps"]), st, K, S, scale)
            reasons["shadow-step"][sel] |= ambiguous
        else:
            light = np.ones(len(sel))
        colour = smoke_color(raw, soot, humidity, temperature, age, st, K)
        albedo = np.clip(st["scattering"] / (st["scattering"] + st["absorption"] + soot * K["albedo_soot"] + K["albedo_eps"]), K["albedo_lo"], K["albedo_hi"])
        sigma_s = sigma_t * albedo
        sky = sky_colour * ((K["sky_base"] + K["sky_shadow"] * np.clip(1.0 - light, 0.0, 1.0)) * np.clip(1.0 - soot * K["sky_soot"], K["sky_soot_lo"], 1.0))[:, None]
        bounce = bounce_colour * np.clip(1.0 - (p[:, 1] - floor_y) / height_scale, 0.0, 1.0)[:, None]
        powder = np.clip(1.0 - np.exp(-sigma_t * step * K["powder_depth"]), 0.0, 1.0) * K["powder_gain"] * np.sqrt(light)
        ph = phase(cos_theta[sel], st["phase_g"], K)
        scattered = colour * sigma_s[:, None] * (sun_radiance * (ph * light)[:, None] + sky + bounce + powder[:, None])
        freshness = np.clip(1.0 - age / K["fire_fresh"], 0.0, 1.0)
        fire = fire_colour * np.clip((temperature * freshness * freshness * K["fire_heat"] + emission * K["fire_emission"]) * st["fire_glow"], 0.0, K["fire_clamp"])[:, None]
        rgb[sel] += (scattered + fire) * (seg_weight * trans[sel])[:, None]
        trans[sel] *= seg_trans
        reasons["opacity-cut"][sel] |= np.abs(trans[sel] - K["opacity_cut"]) < BAND_CUT * K["opacity_cut"]

    alpha = np.clip(1.0 - trans, 0.0, 1.0)
    reasons["unpremultiply"] = np.abs(alpha - K["alpha_switch"]) < BAND_ALPHA
    straight = np.where((alpha > K["alpha_switch"])[:, None], rgb / np.maximum(alpha, 1e-300)[:, None], rgb) * st["exposure"]
    mapped = straight / (K["tone_knee"] + straight)
    shape = (height, width)
    reasons = {name: m.reshape(shape) for name, m in reasons.items()}
    return dict(rgb=mapped.reshape(shape + (3,)), alpha=alpha.reshape(shape), transmittance=trans.reshape(shape), steps=steps.reshape(shape),
                reasons=reasons, masked=np.logical_or.reduce(list(reasons.values())), faint=(alpha < ALPHA_FLOOR).reshape(shape))


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def channels(image):
    """The five compared channels of a float result (a `render` dict or smoke_oracle.hook_march's), as float64 (h, w) arrays."""
    rgb = np.asarray(image["rgb"], f64)
    return {"r": rgb[..., 0], "g": rgb[..., 1], "b": rgb[..., 2], "alpha": np.asarray(image["alpha"], f64), "transmittance": np.asarray(image["transmittance"], f64)}


def masked_share(want):
    """The share of the pixels with reference alpha above the floor that the masks leave out (held to MASK_CAP)."""
    solid = ~want["faint"]
    return float((want["masked"] & solid).sum()) / max(1, int(solid.sum()))


def residuals(got, want):
    """Per channel, the largest |got - want| outside the masks in eps32 * max|want|; the colour of faint pixels is compared
    premultiplied (colour * alpha on both sides).  Also "steps": the number of unmasked pixels whose step counts differ."""
    g, w = channels(got), channels(want)
    keep, faint = ~want["masked"], want["faint"]
    out = {}
    for ch in CHANNELS:
        a, b = g[ch], w[ch]
        if ch in "rgb":
            a, b = np.where(faint, a * g["alpha"], a), np.where(faint, b * w["alpha"], b)
        top = float(np.abs(w[ch]).max())
        out[ch] = float(np.abs(a - b)[keep].max()) / (EPS32 * top) if keep.any() and top > 0.0 else float(np.abs(a - b)[keep].max() if keep.any() else 0.0)
    step_keep = keep & ~want["reasons"]["step-count"]
    out["steps"] = int((np.asarray(got["steps"]) != want["steps"])[step_keep].sum())
    return out


def code_gates(name, want):
    """Per 8-bit channel (r, g, b, alpha): G = 255 * gate * eps32 * max|reference|, the share of a code the float gate is worth."""
    w = channels(want)
    return {ch: 255.0 * gate(name, ch) * EPS32 * float(np.abs(w[ch]).max()) for ch in ("r", "g", "b", "alpha")}


def code_residuals(rgba, want):
    """An RGBA8 image against the reference: per channel (worst |code - 255 v_ref| outside the masks, |mean(code - 255 v_ref)|
    over the unmasked pixels above the floor, their number).  Faint pixels' colour is compared premultiplied."""
    w = channels(want)
    keep, faint = ~want["masked"], want["faint"]
    code = np.asarray(rgba, f64)
    a_code = code[..., 3] / 255.0
    out = {}
    for i, ch in enumerate(("r", "g", "b", "alpha")):
        a, b = code[..., i], 255.0 * w[ch]
        if ch != "alpha":
            a, b = np.where(faint, a * a_code, a), np.where(faint, b * w["alpha"], b)
        d = a - b
        solid = keep & ~faint
        out[ch] = (float(np.abs(d[keep]).max()) if keep.any() else 0.0, abs(float(d[solid].mean())) if solid.any() else 0.0, int(solid.sum()))
    return out


def hold_codes(name, tag, rgba, want):
    """Assert the 8-bit gate and the bias gate of an image (the host's oracle images and the device's)."""
    G = code_gates(name, want)
    for ch, (worst, bias, count) in code_residuals(rgba, want).items():
        print(f"smoke-march-code {tag:10s} {name:18s} {ch:6s} worst {worst:6.3f} (gate {0.5 + G[ch]:.4f})   bias {bias:7.4f} (gate {2.0 / math.sqrt(max(count, 1)) + G[ch]:.4f}, {count} pixels)")
        assert worst <= 0.5 + G[ch], (name, tag, ch, worst, 0.5 + G[ch])
        if count:
            assert bias <= 4.0 * 0.5 / math.sqrt(count) + G[ch], (name, tag, ch, bias, count)
