"""An independent float64 NumPy statement of the clearance rasters' contract (csrc/f3d_clearance.h) -- TEST INFRASTRUCTURE ONLY.

The first form of L*, from the SAMPLE: for one observer (x, Y, z, w) and every sample of a region the line
p(t) = (g.x + t dx, g.z + t dz), t in (0, 1), is cut at its crossings with EVERY lattice line up to the observer or the
footprint's exit (no pyramid, no pruning, no walk); on each segment between two crossings the numerator
Q(t) = y(p(t)) - t Y - h (1 - t) is a quadratic, fitted through three exact evaluations of the cell's bilinear surface (both
ends and the middle); the maximum of Q(t) / (1 - t) + k t over the segment is at an end or at its stationary point.  L* is
the maximum over the segments, and the raster's value max(L*, 0); no segment: 0.

What the contract fixes in float32 is taken in float32 and promoted: the lattice (line X of the x axis is
fma(X, spacing_x, origin_x)), the sample's height, dx = x - g.x and dz = z - g.z, hd2 = dx dx + dz dz (two products, one
sum: the distance cut-off and hd2 == 0 are decided on it) and k = hd2 inv_two_r_prime.  Everything after that is float64.
`dense_clearance` is the brute force this form is checked against (tests/test_session_clearance_host.py).
"""
from __future__ import annotations

import numpy as np

from horizon_reference import Surface  # noqa: F401  (the terrain as a session holds it, and its lattice)

f32, f64 = np.float32, np.float64


def _crossings(lines, idx, d):
    """Parameters at which the lines from lines[idx] along d (n,) cross the lattice lines ahead (n, M), inf where there is
    none, and the parameter of the last one (0: none ahead; inf: the line does not move along this axis and has cells beside
    it -- along a lattice line it lies in the cells on the higher-index side, none along the last line)."""
    m = len(lines)
    step = np.arange(1, m)
    sign = np.where(d > 0, 1, -1)
    tgt = idx[:, None] + sign[:, None] * step[None, :]
    valid = (tgt >= 0) & (tgt < m) & (d != 0)[:, None]
    with np.errstate(all="ignore"):
        t = np.where(valid, (lines[np.clip(tgt, 0, m - 1)] - lines[idx][:, None]) / np.where(d != 0, d, 1.0)[:, None], np.inf)
    last = np.where(valid, t, 0.0).max(axis=1)
    return t, np.where(d != 0, last, np.where(idx < m - 1, np.inf, 0.0))


def sample_geometry(surface, region, observer, inv_two_r_prime, curved):
    """What the contract computes in float32 for every sample of the region, promoted: jj, ii, g.x, h, g.z, dx, dz, hd2, k."""
    row0, col0, rows, cols = region
    jj, ii = (a.reshape(-1) for a in np.meshgrid(np.arange(row0, row0 + rows), np.arange(col0, col0 + cols), indexing="ij"))
    x, _, z, _ = (f32(v) for v in observer)
    gx, gz, h = surface.X[ii], surface.Z[jj], surface.h64[jj, ii]
    dx = (x - gx.astype(f32)).astype(f32)
    dz = (z - gz.astype(f32)).astype(f32)
    hd2 = (dx * dx + dz * dz).astype(f32)
    k = (hd2 * f32(inv_two_r_prime)).astype(f32).astype(f64) if curved else np.zeros(len(ii))
    return jj, ii, gx, h, gz, dx.astype(f64), dz.astype(f64), hd2, k


def clearance_reference(surface, region, observer, inv_two_r_prime=0.0, curved=False, return_between=False):
    """float64 (rows, cols): the contract's value for every sample of `region` and one observer (x, Y, z, w) float32.
    return_between: also the bool raster "some terrain lies between" (a walk takes place and meets a cell)."""
    rows, cols = region[2], region[3]
    jj, ii, gx, h, gz, dx, dz, hd2, k = sample_geometry(surface, region, observer, inv_two_r_prime, curved)
    Y, w = f64(f32(observer[1])), f32(observer[3])
    tx, x_exit = _crossings(surface.X, ii, dx)
    tz, z_exit = _crossings(surface.Z, jj, dz)
    t_end = np.minimum(np.minimum(x_exit, z_exit), 1.0)
    n = len(ii)
    ts = np.sort(np.concatenate([np.zeros((n, 1)), np.ones((n, 1)), tx, tz], axis=1), axis=1)
    ta, tb = ts[:, :-1], ts[:, 1:]
    with np.errstate(all="ignore"):
        # (a line through a lattice corner crosses its two lines at parameters that may differ in the last place: such a sliver
        # has no room for a three-point fit and nothing to add -- the surface is continuous and its neighbours hold both ends)
        ok = np.isfinite(tb) & (tb - ta > 1e-12) & (tb <= t_end[:, None])
        ta, tb = np.where(ok, ta, 0.25), np.where(ok, tb, 0.5)
        tm = 0.5 * (ta + tb)
        px, pz = gx[:, None] + tm * dx[:, None], gz[:, None] + tm * dz[:, None]
        cx = np.clip(np.searchsorted(surface.X, px, side="right") - 1, 0, surface.cols - 2)
        cz = np.clip(np.searchsorted(surface.Z, pz, side="right") - 1, 0, surface.rows - 2)

        def Q(t):
            y = surface.height_in(cx, cz, gx[:, None] + t * dx[:, None], gz[:, None] + t * dz[:, None])
            return y - t * Y - h[:, None] * (1.0 - t)

        f0, fm, f1 = Q(ta), Q(tm), Q(tb)
        half = 0.5 * (tb - ta)
        a = (f0 - 2.0 * fm + f1) / (2.0 * half * half)  # Q = a (t - ta)^2 + b (t - ta) + f0
        b = (-3.0 * f0 + 4.0 * fm - f1) / (2.0 * half)
        # in s = 1 - t:  Q = q2 s^2 + q1 s + q0,  f = q0 / s + (q1 + k) + (q2 - k) s
        sa, sb = 1.0 - ta, 1.0 - tb
        q2, q1, q0 = a, -(2.0 * a * sa + b), a * sa * sa + b * sa + f0
        q0 = np.where(tb == 1.0, f1, q0)  # (Q at the observer: evaluated, not continued)
        kk = k[:, None]
        f = lambda s: q0 / s + (q1 + kk) + (q2 - kk) * s
        at_a = f(sa)
        at_b = np.where(sb > 0.0, f(np.where(sb > 0.0, sb, 1.0)), np.where(q0 > 0.0, np.inf, np.where(q0 < 0.0, -np.inf, q1 + kk)))
        best = np.maximum(at_a, at_b)
        den = q2 - kk
        ratio = np.where(den != 0.0, q0 / np.where(den != 0.0, den, 1.0), -1.0)
        star = np.sqrt(np.where(ratio > 0.0, ratio, 1.0))
        inside = (ratio > 0.0) & (star > sb) & (star < sa)
        best = np.where(inside, np.maximum(best, f(star)), best)
        lstar = np.where(ok, best, -np.inf).max(axis=1)
    between = ok.any(axis=1)
    out = np.maximum(lstar, 0.0)
    zero = hd2 == 0
    out = np.where(zero, np.where(Y < h, np.inf, 0.0), out)
    between = between & ~zero
    if w > 0:
        cut = hd2 > w * w
        out = np.where(cut, np.inf, out)
        between = between & ~cut
    out = out.reshape(rows, cols)
    return (out, between.reshape(rows, cols)) if return_between else out


def dense_clearance(surface, sample, observer, inv_two_r_prime=0.0, curved=False, samples_per_cell=4000):
    """Brute force for ONE sample (j, i) and one observer (no distance limit, hd2 > 0): the maximum of the first form over a
    dense set of parameters in (0, 1) inside the footprint, clamped at 0."""
    j, i = sample
    _, _, gx, h, gz, dx, dz, _, k = sample_geometry(surface, (j, i, 1, 1), observer, inv_two_r_prime, curved)
    Y = f64(f32(observer[1]))
    _, x_exit = _crossings(surface.X, np.array([i]), dx)
    _, z_exit = _crossings(surface.Z, np.array([j]), dz)
    t_end = min(x_exit[0], z_exit[0], 1.0)
    if not t_end > 0.0:
        return 0.0
    t = np.linspace(0.0, t_end, samples_per_cell * (surface.rows + surface.cols))[1:]
    t = t[t < 1.0]
    y = surface.height(gx[0] + t * dx[0], gz[0] + t * dz[0])
    return max(float(((y - t * Y) / (1.0 - t) + k[0] * t - h[0]).max()), 0.0)
