"""An independent float64 NumPy statement of the shadow-depth rasters' contract (csrc/f3d_umbra.h) -- TEST INFRASTRUCTURE ONLY.

For one direction (dx, dy, dz, w) and every sample of a region: the line p(t) = (g.x + t dx, g.z + t dz) is cut at its crossings
with EVERY lattice line up to the footprint's exit (no pyramid, no pruning, no walk); on each segment between two crossings the
functional f(t) = y(p(t)) - k t^2 - dy t - h is a quadratic, fitted through three exact evaluations of the cell's bilinear
surface (both ends and the middle); its maximum over the segment is at an end or at its vertex.  The value is the maximum over
the segments and +0 (the limit t -> 0+); no segment: exactly 0.

The lattice is the one the library steps over (horizon_reference.Surface: line X of the x axis is float32
fma(X, spacing_x, origin_x), promoted), the sample's height and the direction are float32, promoted; everything after that is
float64.  `dense_umbra` is the brute force this form is checked against (tests/test_session_umbra_host.py).
"""
from __future__ import annotations

import numpy as np

from horizon_reference import Surface, _crossings, curvature_k  # noqa: F401  (the terrain as a session holds it, its lattice)

f32, f64 = np.float32, np.float64


def special_value(direction):
    """The contract's special values of a direction (4,), in its order: NaN, 0.0, inf -- or None: a walk takes place."""
    dx, dy, dz, w = (f32(v) for v in direction)
    if not (np.isfinite(dx) and np.isfinite(dy) and np.isfinite(dz) and w == 0.0):
        return np.nan
    if dx == 0.0 and dz == 0.0:
        return 0.0 if dy > 0.0 else (np.inf if dy < 0.0 else np.nan)
    return None


def umbra_reference(surface, region, direction, inv_two_r_prime=0.0, curved=False, return_along=False):
    """float64 (rows, cols): the contract's value for every sample of `region` and one direction (dx, dy, dz, w) float32.
    return_along: also the bool raster "some terrain lies along the direction" (a walk takes place and meets a cell)."""
    row0, col0, rows, cols = region
    special = special_value(direction)
    if special is not None:
        out = np.full((rows, cols), special, f64)
        return (out, np.zeros((rows, cols), bool)) if return_along else out
    jj, ii = (a.reshape(-1) for a in np.meshgrid(np.arange(row0, row0 + rows), np.arange(col0, col0 + cols), indexing="ij"))
    gx, gz, h = surface.X[ii], surface.Z[jj], surface.h64[jj, ii]
    dx, dy, dz = (f64(f32(v)) for v in direction[:3])
    k = curvature_k((dx, dz), inv_two_r_prime, curved)
    tx, x_exit = _crossings(surface.X, ii, dx)
    tz, z_exit = _crossings(surface.Z, jj, dz)
    t_exit = np.minimum(x_exit, z_exit)
    ts = np.sort(np.concatenate([np.zeros((len(ii), 1)), tx, tz], axis=1), axis=1)
    ta, tb = ts[:, :-1], ts[:, 1:]
    with np.errstate(all="ignore"):
        # (a line through a lattice corner crosses its two lines at parameters that may differ in the last place: such a sliver
        # has no room for a three-point fit and nothing to add -- the surface is continuous and its neighbours hold both ends)
        ok = np.isfinite(tb) & (tb - ta > 1e-9 * tb) & (tb <= t_exit[:, None])
        ta, tb = np.where(ok, ta, 1.0), np.where(ok, tb, 2.0)
        tm = 0.5 * (ta + tb)
        cx = np.clip(np.searchsorted(surface.X, gx[:, None] + tm * dx, side="right") - 1, 0, surface.cols - 2)
        cz = np.clip(np.searchsorted(surface.Z, gz[:, None] + tm * dz, side="right") - 1, 0, surface.rows - 2)
        f0, fm, f1 = (surface.height_in(cx, cz, gx[:, None] + t * dx, gz[:, None] + t * dz) - k * t * t - dy * t - h[:, None] for t in (ta, tm, tb))
        half = 0.5 * (tb - ta)
        a = (f0 - 2.0 * fm + f1) / (2.0 * half * half)  # f = a (t - ta)^2 + b (t - ta) + f0
        b = (-3.0 * f0 + 4.0 * fm - f1) / (2.0 * half)
        best = np.maximum(f0, f1)
        s = np.where(a < 0.0, -b / np.where(a < 0.0, 2.0 * a, 1.0), -1.0)
        inside = (a < 0.0) & (s > 0.0) & (s < 2.0 * half)
        best = np.where(inside, np.maximum(best, f0 + 0.5 * b * s), best)
        sup = np.where(ok, best, -np.inf).max(axis=1)
    along = ok.any(axis=1).reshape(rows, cols)
    out = np.maximum(sup, 0.0).reshape(rows, cols)
    return (out, along) if return_along else out


def dense_umbra(surface, sample, direction, inv_two_r_prime=0.0, curved=False, samples_per_cell=4000):
    """Brute force for ONE sample (j, i) and one direction with a horizontal part: the maximum of the functional over a dense
    set of parameters inside the footprint, clamped at 0."""
    j, i = sample
    dx, dy, dz = (f64(f32(v)) for v in direction[:3])
    k = curvature_k((dx, dz), inv_two_r_prime, curved)
    gx, gz, h = surface.X[i], surface.Z[j], surface.h64[j, i]
    _, x_exit = _crossings(surface.X, np.array([i]), dx)
    _, z_exit = _crossings(surface.Z, np.array([j]), dz)
    t_exit = min(x_exit[0], z_exit[0])
    if not t_exit > 0.0:
        return 0.0
    t = np.linspace(0.0, t_exit, samples_per_cell * (surface.rows + surface.cols))[1:]
    return max(float((surface.height(gx + t * dx, gz + t * dz) - k * t * t - dy * t - h).max()), 0.0)
