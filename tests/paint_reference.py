"""An independent float64 statement of the paint contract (csrc/f3d_paint.h) -- TEST INFRASTRUCTURE ONLY.

NumPy, every texel against every primitive, no tiles, no f32: what tests/test_session_paint_host.py holds the host build of the
lane body to.  Inputs are the f32 values the library is given (vertices, colours, the DEM's frame, the drape's registration),
taken to float64 exactly; everything after that is float64.

The two tolerances of the host tests are written down here:

* ``COVERAGE_TOL`` -- stroke coverage (and the lerp parameter where coverage is positive), host f32 body against this file:
  8 x the largest difference measured on the tests' own inputs (SCENES of tests/test_session_paint_host.py: a 33x33 DEM at 10 m
  under a 70x130 canvas and the anisotropic 33x17 one under 257x64, vertices uniform in +-170 m, half-widths 0 .. 25 m).  The
  difference is the rounding of d = |p - a - t e| (relative 2^-24 per operation on lengths up to ~500 m, so ~1e-4 m) divided by
  the ramp (2.3 m and more): the measured maximum is one draw of that, and 8 x it the margin the raster tests use.
* ``BLEND_TOL`` -- blended values before they are rounded to binary16: the coverage error times opacity x alpha x |src - dst| <= 1,
  plus the lerp's and the blend's own roundings (2^-24 each on values in [0, 1]), again 8 x the measured maximum.  Stored
  texels are compared through the half they round to: they may differ by one binary16 step where the f64 value lies within
  BLEND_TOL of a rounding boundary, and by nothing elsewhere.
* ``TRIANGLE_BAND`` -- triangles are 0 / 1, so they are compared as DECISIONS: equal wherever the float64 distance of the texel
  centre to the triangle's nearest edge line exceeds the band.  The f32 edge function (q.x - p.x)(s.z - p.z) - (q.z - p.z)(s.x - p.x)
  of coordinates in +-170 m carries four roundings of relative 2^-24 on terms up to |e| |s - p|, so its error as a distance
  (divided by |e|) is at most ~4 x 2^-24 x 480 m = 1.2e-4 m; the band is 8 x that, rounded: 1e-3 m.  At most 0.5 % of a case's
  texels may lie inside the band (the tests assert it; the scenes have a few per million).
"""
from __future__ import annotations

import numpy as np

POINTS, LINES, TRIANGLES = 0, 1, 2

COVERAGE_MEASURED = 9.95e-6  # max |cov_f32 - cov_f64| over the tests' scenes (test_stroke_coverage_against_the_reference prints each
                             # case's: 6.63e-6 on the square scene, 9.94e-6 on the anisotropic one)
COVERAGE_TOL = 8.0 * COVERAGE_MEASURED
BLEND_MEASURED = 4.74e-6     # max |blend_f32 - blend_f64| per channel, before the rounding to binary16 (test_blended_values_against_the_reference
                             # prints each case's: the anisotropic scene's points)
BLEND_TOL = 8.0 * BLEND_MEASURED
TRIANGLE_BAND = 1.0e-3       # metres
TRIANGLE_BAND_MAX_FRACTION = 0.005

f64 = np.float64


def ramp(frame):
    """One texel in metres: max(|spacing_x / scale_x|, |spacing_z / scale_z|).  frame = (origin_x, origin_z, spacing_x, spacing_z,
    scale_x, offset_x, scale_z, offset_z)."""
    ox, oz, sx, sz, kx, bx, kz, bz = (f64(v) for v in frame)
    return max(abs(sx / kx), abs(sz / kz))


def centres(rows, cols, frame):
    """World (x, z) of every texel centre, (rows, cols) each: the inverse of the drape's registration."""
    ox, oz, sx, sz, kx, bx, kz, bz = (f64(v) for v in frame)
    x = ox + (np.arange(cols, dtype=f64) - bx) / kx * sx
    z = oz + (np.arange(rows, dtype=f64) - bz) / kz * sz
    return np.broadcast_to(x[None, :], (rows, cols)), np.broadcast_to(z[:, None], (rows, cols))


def segment(a, b, half_width, one_texel, x, z):
    """(cov, t, d) of the stroke (a, b) at the points (x, z)."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    e = b - a
    qx, qz = x - a[0], z - a[1]
    den = e @ e
    t = np.zeros_like(x) if den == 0.0 else np.clip((qx * e[0] + qz * e[1]) / den, 0.0, 1.0)
    d = np.hypot(qx - t * e[0], qz - t * e[1])
    return np.clip((half_width - d) / one_texel + 0.5, 0.0, 1.0), t, d


def _cross(p, q, x, z):
    return (q[0] - p[0]) * (z - p[1]) - (q[1] - p[1]) * (x - p[0])


def triangle(v, x, z):
    """(inside, b1, b2, edge_distance) of the triangle v (3 x 2) at the points (x, z): inside by the sign of the three cross
    products in the triangle's positive winding, zeros to the edges with dz > 0 or (dz == 0 and dx < 0); edge_distance = the
    distance to the nearest of the three edge LINES (how far a texel is from changing its decision)."""
    v = np.asarray(v, f64)
    area = _cross(v[0], v[1], v[2, 0], v[2, 1])
    if area == 0.0:
        return np.zeros(x.shape, bool), np.zeros_like(x), np.zeros_like(x), np.full(x.shape, np.inf)
    o = 1.0 if area > 0 else -1.0
    inside = np.ones(x.shape, bool)
    w, dist = [], np.full(x.shape, np.inf)
    for p, q in ((v[1], v[2]), (v[2], v[0]), (v[0], v[1])):
        wi = o * _cross(p, q, x, z)
        dx, dz = o * (q[0] - p[0]), o * (q[1] - p[1])
        owns = dz > 0 or (dz == 0 and dx < 0)
        inside &= (wi > 0) | ((wi == 0) & owns)
        dist = np.minimum(dist, np.abs(wi) / np.hypot(dx, dz))
        w.append(wi)
    total = w[0] + w[1] + w[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        b1, b2 = np.where(inside, w[1] / total, 0.0), np.where(inside, w[2] / total, 0.0)
    return inside, b1, b2, dist


def feature_runs(first_vertex_ids):
    """The run number of every primitive: consecutive primitives whose first vertices carry one id are one feature."""
    ids = np.asarray(first_vertex_ids)
    return np.concatenate([[0], np.cumsum(ids[1:] != ids[:-1])]).astype(np.int64) if len(ids) else np.zeros(0, np.int64)


def paint(values, frame, xz, rgba, indices, kind, half_width, opacity, features=None):
    """The canvas after one call, float64 (rows, cols, 3), NOT rounded to binary16.  values: (rows, cols, 3), what the texels hold;
    xz (N, 2), rgba (N, 4), indices flat (1 / 2 / 3 a primitive), features (N,) ids or None."""
    dst = np.array(values, f64)
    rows, cols = dst.shape[:2]
    x, z = centres(rows, cols, frame)
    xz, rgba = np.asarray(xz, f64), np.asarray(rgba, f64)
    per = kind + 1
    prims = np.asarray(indices, np.int64).reshape(-1, per)
    runs = feature_runs(np.asarray(features)[prims[:, 0]]) if features is not None else np.zeros(len(prims), np.int64)
    one_texel = ramp(frame)
    best = np.zeros((rows, cols))
    src = np.zeros((rows, cols, 4))

    def flush():
        a = (f64(opacity) * src[..., 3] * best)[..., None]
        return dst + a * (src[..., :3] - dst)

    for i, prim in enumerate(prims):
        if i > 0 and runs[i] != runs[i - 1]:
            dst = flush()
            best = np.zeros((rows, cols))
        if kind == TRIANGLES:
            inside, b1, b2, _ = triangle(xz[prim], x, z)
            cov = inside.astype(f64)
            c0, c1, c2 = rgba[prim[0]], rgba[prim[1]], rgba[prim[2]]
            colour = c0 + b1[..., None] * (c1 - c0) + b2[..., None] * (c2 - c0)
        else:
            a, b = xz[prim[0]], xz[prim[-1]]
            cov, t, _ = segment(a, b, f64(half_width), one_texel, x, z)
            colour = rgba[prim[0]] + t[..., None] * (rgba[prim[-1]] - rgba[prim[0]])
        take = cov > best  # ties go to the lowest index
        best = np.where(take, cov, best)
        src = np.where(take[..., None], colour, src)
    return flush()
