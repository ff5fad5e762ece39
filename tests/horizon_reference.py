"""An independent float64 NumPy statement of the horizon rasters' contract (csrc/f3d_horizon.h) -- TEST INFRASTRUCTURE ONLY.

For one azimuth (dx, dz) and every sample of a region: the line p(t) = (o.x + t dx, o.z + t dz) is cut at its crossings with
EVERY lattice line up to the footprint's exit (no pyramid, no pruning, no walk); on each segment between two crossings the
function f(t) = y(p(t)) - k t^2 - o.y is a quadratic, fitted through three exact evaluations of the cell's bilinear surface
(both ends and the middle); the maximum of f(t) / t = A t + B + C / t over the segment is at an end or at sqrt(C / A).  The
horizon is the maximum over the segments, -inf without one.

The lattice is the one the library steps over: line X of the x axis is float32 fma(X, spacing_x, origin_x), promoted to
float64 -- so a sample lies exactly on its own two lines -- and o.y is the float32 sum h + lift.  Everything after that is
float64.  `dense_horizon` is the brute force this form is checked against (tests/test_session_horizon_host.py).
"""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64


def lattice(origin, spacing, count):
    """float64 values of the float32 lattice lines 0 .. count - 1 (f3d_trace.h plane_at: one rounding)."""
    return (np.arange(count, dtype=f64) * f64(spacing) + f64(origin)).astype(f32).astype(f64)


def curvature_k(direction, inv_two_r_prime, curved):
    dx, dz = f64(direction[0]), f64(direction[1])
    return (dx * dx + dz * dz) * f64(inv_two_r_prime) if curved else 0.0


class Surface:
    """The terrain as a session holds it: float32 heights times the exaggeration (one float32 product), its lattice."""

    def __init__(self, dem, exaggeration, origin, spacing):
        self.h = (np.asarray(dem, f32) * f32(exaggeration)).astype(f32)
        self.rows, self.cols = self.h.shape
        self.X, self.Z = lattice(origin[0], spacing[0], self.cols), lattice(origin[1], spacing[1], self.rows)
        self.h64 = self.h.astype(f64)

    def origins_y(self, jj, ii, lift):
        return (self.h[jj, ii] + f32(lift)).astype(f32).astype(f64)

    def height(self, px, pz):
        """Bilinear surface of the cell under (px, pz) (points on a line or corner: either neighbour, the surface is continuous)."""
        cx = np.clip(np.searchsorted(self.X, px, side="right") - 1, 0, self.cols - 2)
        cz = np.clip(np.searchsorted(self.Z, pz, side="right") - 1, 0, self.rows - 2)
        return self.height_in(cx, cz, px, pz)

    def height_in(self, cx, cz, px, pz):
        u = (px - self.X[cx]) / (self.X[cx + 1] - self.X[cx])
        v = (pz - self.Z[cz]) / (self.Z[cz + 1] - self.Z[cz])
        h = self.h64
        return (h[cz, cx] * (1 - u) + h[cz, cx + 1] * u) * (1 - v) + (h[cz + 1, cx] * (1 - u) + h[cz + 1, cx + 1] * u) * v


def _crossings(lines, idx, d):
    """Parameters at which the line from lines[idx] crosses the lattice lines ahead (n, M), inf where there is none, and the
    parameter of the last one (0: none ahead; inf: the line does not move along this axis and has cells beside it)."""
    n = len(idx)
    if d == 0.0:  # (along a lattice line: in the cells on its higher-index side, none along the last line -- the contract's footprint)
        return np.full((n, 0), np.inf), np.where(idx < len(lines) - 1, np.inf, 0.0)
    step = np.arange(1, len(lines))
    tgt = idx[:, None] + (1 if d > 0 else -1) * step[None, :]
    valid = (tgt >= 0) & (tgt < len(lines))
    t = np.where(valid, (lines[np.clip(tgt, 0, len(lines) - 1)] - lines[idx][:, None]) / d, np.inf)
    return t, np.where(valid, t, 0.0).max(axis=1)


def horizon_reference(surface, region, lift, azimuths, inv_two_r_prime=0.0, curved=False, return_exit=False):
    """float64 (K, rows, cols): the contract's H for every sample of `region` and every azimuth of `azimuths` (K, 2) float32."""
    row0, col0, rows, cols = region
    jj, ii = (a.reshape(-1) for a in np.meshgrid(np.arange(row0, row0 + rows), np.arange(col0, col0 + cols), indexing="ij"))
    oy = surface.origins_y(jj, ii, lift)
    ox, oz = surface.X[ii], surface.Z[jj]
    out, exits = [], []
    for direction in np.asarray(azimuths, f32).reshape(-1, 2):
        dx, dz = f64(direction[0]), f64(direction[1])
        k = curvature_k(direction, inv_two_r_prime, curved)
        tx, x_exit = _crossings(surface.X, ii, dx)
        tz, z_exit = _crossings(surface.Z, jj, dz)
        t_exit = np.minimum(x_exit, z_exit)
        ts = np.sort(np.concatenate([np.zeros((len(ii), 1)), tx, tz], axis=1), axis=1)
        ta, tb = ts[:, :-1], ts[:, 1:]
        with np.errstate(all="ignore"):
            ok = np.isfinite(tb) & (tb > ta) & (tb <= t_exit[:, None])
            ta, tb = np.where(ok, ta, 1.0), np.where(ok, tb, 2.0)
            tm = 0.5 * (ta + tb)
            cx = np.clip(np.searchsorted(surface.X, ox[:, None] + tm * dx, side="right") - 1, 0, surface.cols - 2)
            cz = np.clip(np.searchsorted(surface.Z, oz[:, None] + tm * dz, side="right") - 1, 0, surface.rows - 2)
            f0, fm, f1 = (surface.height_in(cx, cz, ox[:, None] + t * dx, oz[:, None] + t * dz) - k * t * t - oy[:, None] for t in (ta, tm, tb))
            half = 0.5 * (tb - ta)
            a = (f0 - 2.0 * fm + f1) / (2.0 * half * half)
            b = (-3.0 * f0 + 4.0 * fm - f1) / (2.0 * half)
            A, B, C = a, b - 2.0 * a * ta, f0 - b * ta + a * ta * ta  # (in t; the fit was in t - ta)
            C = np.where(ta == 0.0, f0, C)
            g = lambda t: A * t + B + C / t
            at_start = np.where(ta > 0.0, g(np.where(ta > 0.0, ta, 1.0)), np.where(C < 0.0, -np.inf, np.where(C > 0.0, np.inf, B)))
            best = np.maximum(at_start, g(tb))
            ratio = np.where(A != 0.0, C / np.where(A != 0.0, A, 1.0), -1.0)
            star = np.sqrt(np.where(ratio > 0.0, ratio, 1.0))
            inside = (ratio > 0.0) & (star > ta) & (star < tb)
            best = np.where(inside, np.maximum(best, g(star)), best)
            out.append(np.where(ok, best, -np.inf).max(axis=1).reshape(rows, cols))
        exits.append(t_exit.reshape(rows, cols))
    return (np.stack(out), np.stack(exits)) if return_exit else np.stack(out)


def dense_horizon(surface, sample, lift, direction, samples_per_cell=4000, k=0.0):
    """Brute force for ONE sample (j, i) and one azimuth: the maximum of f(t) / t over a dense set of parameters in the footprint."""
    j, i = sample
    dx, dz = f64(direction[0]), f64(direction[1])
    oy = surface.origins_y(np.array([j]), np.array([i]), lift)[0]
    ox, oz = surface.X[i], surface.Z[j]
    _, x_exit = _crossings(surface.X, np.array([i]), dx)
    _, z_exit = _crossings(surface.Z, np.array([j]), dz)
    t_exit = min(x_exit[0], z_exit[0])
    if not t_exit > 0.0:
        return -np.inf
    t = np.linspace(0.0, t_exit, samples_per_cell * (surface.rows + surface.cols))[1:]
    return float(((surface.height(ox + t * dx, oz + t * dz) - k * t * t - oy) / t).max())


def sky_view_f32(planes, azimuths):
    """The stated sky-view formula from returned planes (K, ...), float32 with one rounding per operation, summed for k = 0, 1, ..."""
    planes = np.asarray(planes, f32)
    total = np.zeros(planes.shape[1:], f32)
    with np.errstate(all="ignore"):
        for H, (dx, dz) in zip(planes, np.asarray(azimuths, f32).reshape(-1, 2)):
            h = H / np.sqrt(dx * dx + dz * dz)
            total = total + np.where(h > 0.0, h / np.sqrt(f32(1.0) + h * h), f32(0.0)).astype(f32)
        out = f32(1.0) - total / f32(len(planes))
    assert out.dtype == f32
    return out
