"""An independent float64 NumPy statement of the ray query's geometry (csrc/f3d_march.h, f3d_query.h, f3d_raster.h) -- TEST
INFRASTRUCTURE ONLY.  Nothing here comes from oracle/, tests/emul or the kernel headers: no pyramid, no stack, no slab test.

Terrain.  For one ray (o, tmin, d, tmax) and k = (dx^2 + dz^2) inv_two_r_prime (0 when the curvature policy is off) the
interval [tmin, tmax] is clipped to the footprint and cut at its crossings with EVERY lattice line; on each segment

    f(t) = o.y + t d.y + k t^2 - height(p(t))

is exactly quadratic (a bilinear patch along a straight line), fitted through three evaluations: both ends and the middle,
the cell taken from the midpoint.  `first` is the smallest root in (tmin, tmax), inf without one; `clear` the minimum of f
over the clipped interval (ends and vertices), +inf when the ray never passes over the footprint; `normal` the unit normal
of the bilinear patch at `first`.  The lattice is horizon_reference.Surface's: line X is float32 fma(X, spacing, origin)
promoted, heights are the float32 products with the exaggeration.  The rays are taken as float32 and promoted; everything
after that is float64.

A ray that runs exactly along a lattice line (d.x == 0 with o.x on a line, or the same in z) lies in the cells on the line's
higher-index side and in none along the last line -- horizon_reference._crossings' rule, the contract's footprint
[first line, last line).

Mesh.  `triangle_search`: float64 Moeller-Trumbore over all triangles, the reference shader's acceptance (|a| >= 1e-7,
0 <= u <= 1, v >= 0, u + v <= 1, t in (tmin, tmax)).  `mesh_reference`: the nearest t, its triangle, and the ray's smallest
barycentric margin over the triangles it nearly touches.

`dense_trace` is the brute force the segment form is checked against (tests/test_trace_reference_host.py).

The two tolerances of the gates are MEASURED on the oracle, not chosen (tests/test_trace_reference_host.py part b prints
them; the gate is four times the largest value, rounded up to two digits):

    python -m pytest -m "not gpu" tests/test_trace_reference_host.py -k oracle -s | grep "trace-ref"

MEASURED_ON_THE_ORACLE below holds, per set, the largest height residual as a multiple of ulp(max(|o.y|, max height)) and
the largest normal angle in radians.  The host and GPU tests import HEIGHT_TOL_ULPS and ANGLE_TOL_RAD; neither derives a
tolerance from the code it checks.

What the measurement says about the error: the height residual is the float32 rounding of t carried along the ray's slope
and of the leaf's own interpolation, a few ulp of the heights in play on every set (1.8 on the proof DEM, up to 6.8 on the
small shapes, whose rays are steeper against their relief); the normal's angle is the float32 hit position's error times the
patch's twist, and so largest where the cells are roughest (the re-terrained patch).
"""
from __future__ import annotations

import numpy as np

from horizon_reference import Surface  # noqa: F401  (the terrain as a session holds it, and its lattice)

f32, f64 = np.float32, np.float64

# name of the set -> (height residual in ulp(max(|o.y|, max height)), normal angle in radians), the oracle's maxima
MEASURED_ON_THE_ORACLE = {
    "proof": (1.8, 1.3e-8),
    "list-2x2": (2.2, 4.9e-10),
    "list-3x5": (2.5, 1.8e-9),
    "list-63x65": (3.6, 4.2e-7),
    "list-17x130": (6.3, 1.2e-6),
    "list-33x33": (4.1, 2.9e-7),
    "list-64x64": (6.6, 6.2e-7),
    "list-64x64-reterrain": (6.8, 3.6e-6),  # (the golden DEM with a rougher 16x16 patch: steeper, more twisted cells)
}
HEIGHT_TOL_ULPS = {name: 4.0 * v[0] for name, v in MEASURED_ON_THE_ORACLE.items()}
ANGLE_TOL_RAD = {name: 4.0 * v[1] for name, v in MEASURED_ON_THE_ORACLE.items()}

BAND = 1e-5           # the hit/miss gate leaves out |clear| < BAND * relief
BAND_CAP = 0.005      # ... and a set may hold at most this share of such rays
MESH_BAND = 1e-6      # rays whose barycentric margin is under this are left out of the mesh comparison
MESH_BAND_CAP = 0.01
MESH_NEAR = 1e-3      # "nearly touches": the ray's point in the triangle's plane is this close to the triangle


def height_unit(surface, rays):
    """(n,) float64: ulp(max(|o.y|, max height)) in float32, the unit the height tolerance is stated in."""
    top = np.maximum(np.abs(np.asarray(rays, f32)[:, 1]), f32(np.abs(surface.h).max()))
    return np.spacing(top.astype(f32)).astype(f64)


def relief(surface):
    return float(surface.h64.max() - surface.h64.min())


def curvature_k(rays, inv_two_r_prime, curved):
    r = np.asarray(rays, f32).astype(f64)
    return (r[:, 4] ** 2 + r[:, 6] ** 2) * f64(inv_two_r_prime) if curved else np.zeros(len(r))


def _axis_interval(lines, o, d):
    """Parameters between which o + t d lies inside [lines[0], lines[-1]]; a line that does not move along the axis is
    inside for every t when lines[0] <= o < lines[-1] (the rule for a ray along a lattice line), for none otherwise."""
    with np.errstate(all="ignore"):
        t0, t1 = (lines[0] - o) / d, (lines[-1] - o) / d
    still = d == 0.0
    inside = (o >= lines[0]) & (o < lines[-1])
    lo = np.where(still, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    hi = np.where(still, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return lo, hi


def _cells(surface, px, pz):
    cx = np.clip(np.searchsorted(surface.X, px, side="right") - 1, 0, surface.cols - 2)
    cz = np.clip(np.searchsorted(surface.Z, pz, side="right") - 1, 0, surface.rows - 2)
    return cx, cz


def patch_normal(surface, cx, cz, px, pz):
    """float64 unit normals (..., 3) of the bilinear patch of cell (cx, cz) at (px, pz)."""
    h = surface.h64
    wx, wz = surface.X[cx + 1] - surface.X[cx], surface.Z[cz + 1] - surface.Z[cz]
    u, v = (px - surface.X[cx]) / wx, (pz - surface.Z[cz]) / wz
    h00, h10, h01, h11 = h[cz, cx], h[cz, cx + 1], h[cz + 1, cx], h[cz + 1, cx + 1]
    dh_dx = ((h10 - h00) * (1 - v) + (h11 - h01) * v) / wx
    dh_dz = ((h01 - h00) * (1 - u) + (h11 - h10) * u) / wz
    n = np.stack([-dh_dx, np.ones_like(dh_dx), -dh_dz], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def normal_angle(surface, position, normal):
    """(n,) radians between `normal` (n, 3) and the f64 patch normal at `position` (n, 3).  The patch normal jumps across a
    lattice line, and a float32 hit a hair from one may be reported in either cell: within 1e-5 of a cell's width of a line
    the neighbour's normal at the same point is admitted too (the smaller angle counts)."""
    p, got = np.asarray(position, f64), np.asarray(normal, f64)
    got = got / np.linalg.norm(got, axis=1, keepdims=True)
    wx, wz = np.diff(surface.X).max(), np.diff(surface.Z).max()
    best = np.full(len(p), np.inf)
    for sx in (-1e-5, 1e-5):
        for sz in (-1e-5, 1e-5):
            cx, cz = _cells(surface, p[:, 0] + sx * wx, p[:, 2] + sz * wz)
            n = patch_normal(surface, cx, cz, p[:, 0], p[:, 2])
            best = np.minimum(best, np.arctan2(np.linalg.norm(np.cross(n, got), axis=1), (n * got).sum(-1)))
    return best


def deviation(surface, rays, t, inv_two_r_prime=0.0, curved=False):
    """f(t) of each ray at its own parameter t (n,), float64; the cell is the one under the point."""
    r = np.asarray(rays, f32).astype(f64)
    t = np.asarray(t, f64)
    k = curvature_k(rays, inv_two_r_prime, curved)
    px, pz = r[:, 0] + t * r[:, 4], r[:, 2] + t * r[:, 6]
    return r[:, 1] + t * r[:, 5] + k * t * t - surface.height(px, pz)


def _clipped(surface, r):
    """[ta, tb]: [tmin, tmax] clipped to the footprint, and whether anything is left of it."""
    lo_x, hi_x = _axis_interval(surface.X, r[:, 0], r[:, 4])
    lo_z, hi_z = _axis_interval(surface.Z, r[:, 2], r[:, 6])
    ta = np.maximum(r[:, 3], np.maximum(lo_x, lo_z))
    tb = np.minimum(r[:, 7], np.minimum(hi_x, hi_z))
    passes = tb > ta
    return np.where(passes, ta, 0.0), np.where(passes, tb, 1.0), passes


def _window(lines, o, d, ta, tb):
    """First lattice line of each ray's stretch o + [ta, tb] d and how many lines the stretch meets (its ends included)."""
    a, b = o + ta * d, o + tb * d
    first = np.searchsorted(lines, np.minimum(a, b), side="left")
    return first, np.searchsorted(lines, np.maximum(a, b), side="right") - first


def _crossing_parameters(lines, first, count, o, d, ta):
    """(n, max count): the parameters at which each ray meets the lines of its window, ta where it has fewer (or none: d == 0)."""
    idx = first[:, None] + np.arange(max(int(count.max()), 0) if len(count) else 0)[None, :]
    valid = idx < (first + count)[:, None]
    with np.errstate(all="ignore"):
        t = (lines[np.clip(idx, 0, len(lines) - 1)] - o[:, None]) / d[:, None]
    return np.where(valid & np.isfinite(t), t, ta[:, None])


def _terrain_chunk(surface, rays, inv_two_r_prime, curved):
    r = np.asarray(rays, f32).astype(f64)
    n = len(r)
    ox, oy, oz, tmin, dx, dy, dz, tmax = (r[:, c] for c in range(8))
    k = curvature_k(rays, inv_two_r_prime, curved)
    ta, tb, passes = _clipped(surface, r)
    tx = _crossing_parameters(surface.X, *_window(surface.X, ox, dx, ta, tb), ox, dx, ta)
    tz = _crossing_parameters(surface.Z, *_window(surface.Z, oz, dz, ta, tb), oz, dz, ta)
    cuts = np.concatenate([ta[:, None], tb[:, None], tx, tz], axis=1)
    cuts = np.sort(np.clip(cuts, ta[:, None], tb[:, None]), axis=1)
    t0, t1 = cuts[:, :-1], cuts[:, 1:]
    ok = (t1 > t0) & passes[:, None]
    tm = 0.5 * (t0 + t1)
    cx, cz = _cells(surface, ox[:, None] + tm * dx[:, None], oz[:, None] + tm * dz[:, None])
    # the cell's patch, fetched once: its corner heights and its own lattice lines
    h = surface.h64
    h00, h10, h01, h11 = h[cz, cx], h[cz, cx + 1], h[cz + 1, cx], h[cz + 1, cx + 1]
    x_lo, z_lo = surface.X[cx], surface.Z[cz]
    inv_wx, inv_wz = 1.0 / (surface.X[cx + 1] - x_lo), 1.0 / (surface.Z[cz + 1] - z_lo)

    def f(t):
        u, v = (ox[:, None] + t * dx[:, None] - x_lo) * inv_wx, (oz[:, None] + t * dz[:, None] - z_lo) * inv_wz
        y = (h00 * (1 - u) + h10 * u) * (1 - v) + (h01 * (1 - u) + h11 * u) * v
        return oy[:, None] + t * dy[:, None] + k[:, None] * t * t - y

    f0, fm, f1 = f(t0), f(tm), f(t1)
    del h00, h10, h01, h11, x_lo, z_lo, inv_wx, inv_wz
    # in s = (t - t0) / (t1 - t0):  f = a s^2 + b s + c
    a = 2.0 * f1 + 2.0 * f0 - 4.0 * fm
    b = f1 - f0 - a
    with np.errstate(all="ignore"):
        sv = np.where(a != 0.0, -b / np.where(a != 0.0, 2.0 * a, 1.0), -1.0)
        has_vertex = (sv > 0.0) & (sv < 1.0)
        fv = np.where(has_vertex, f0 + 0.5 * b * sv, np.inf)  # (a sv^2 + b sv + c at sv = -b / 2a)
        seg_min = np.minimum(np.minimum(f0, f1), np.where(has_vertex & (a > 0.0), fv, np.inf))
        under0 = f0 <= 0.0
        cross = under0 != (f1 <= 0.0)  # one root in the segment; otherwise two where the vertex lies on the other side of zero
        root_here = ok & (cross | (has_vertex & ((fv <= 0.0) != under0)))
    rows = np.arange(n)
    first = np.full(n, np.inf)
    at = np.zeros(n, np.int64)
    todo = np.nonzero(root_here.any(axis=1))[0]
    while len(todo):  # the first segment with a root, solved for that segment alone; a root ON tmin or tmax does not count
        seg = np.argmax(root_here[todo], axis=1)
        A, B, Cc, F1, SV, one = (q[todo, seg] for q in (a, b, f0, f1, sv, cross))
        with np.errstate(all="ignore"):
            disc = np.maximum(B * B - 4.0 * A * Cc, 0.0)
            q = -0.5 * (B + np.where(B >= 0.0, 1.0, -1.0) * np.sqrt(disc))
            r0 = np.where(A != 0.0, q / np.where(A != 0.0, A, 1.0), np.inf)
            r1 = np.where(q != 0.0, Cc / np.where(q != 0.0, q, 1.0), np.inf)
            slack = 1e-9
            r0 = np.where((r0 >= -slack) & (r0 <= 1.0 + slack), r0, np.inf)
            r1 = np.where((r1 >= -slack) & (r1 <= 1.0 + slack), r1, np.inf)
            s = np.minimum(r0, r1)
            fallback = np.where(one, Cc / np.where(Cc != F1, Cc - F1, 1.0), SV)  # (no root met the slack: rounding at an end)
            s = np.clip(np.where(np.isfinite(s), s, fallback), 0.0, 1.0)
        t_root = t0[todo, seg] + s * (t1[todo, seg] - t0[todo, seg])
        good = (t_root > tmin[todo]) & (t_root < tmax[todo])
        first[todo[good]], at[todo[good]] = t_root[good], seg[good]
        root_here[todo[~good], seg[~good]] = False
        todo = todo[~good]
        todo = todo[root_here[todo].any(axis=1)]
    any_root = np.isfinite(first)
    fx, fz = ox + np.where(any_root, first, 0.0) * dx, oz + np.where(any_root, first, 0.0) * dz
    normal = np.where(any_root[:, None], patch_normal(surface, cx[rows, at], cz[rows, at], fx, fz), 0.0)
    clear = np.where(ok, seg_min, np.inf).min(axis=1)
    head = np.argmax(ok, axis=1)  # the first segment: from the start to the first lattice crossing
    later = ok & (np.arange(ok.shape[1])[None, :] > head[:, None])
    far = np.minimum(np.where(later, seg_min, np.inf).min(axis=1), np.where(passes, f1[rows, head], np.inf))
    start = np.where(passes, f0[rows, head], np.inf)
    cell = np.where(any_root[:, None], np.stack([cx[rows, at], cz[rows, at]], 1), -1)
    return {"first": first, "clear": clear, "clear_far": far, "normal": normal, "start": start, "passes": passes, "cell": cell}


def terrain_reference(surface, rays, inv_two_r_prime=0.0, curved=False, budget=1_500_000):
    """The query's geometry for rays (n, 8) float32 rows (origin xyz, tmin, direction xyz, tmax), float64 throughout:

    first      (n,)   smallest root of f in (tmin, tmax), inf without one
    clear      (n,)   minimum of f over [tmin, tmax] clipped to the footprint, +inf when the ray never passes over it
    clear_far  (n,)   the same minimum from the first lattice crossing on (a raster ray's own lift is not a near miss)
    normal     (n, 3) unit normal of the bilinear patch at `first`, zeros without a root
    start      (n,)   f at the start of the clipped interval (<= 0: the ray starts on or under the surface)
    passes     (n,)   the clipped interval is not empty
    cell       (n, 2) (cx, cz) of the patch at `first`, -1 without a root

    Vectorised over the rays, which are taken in the order of how many lattice lines they cross, `budget` segments at a time."""
    rays = np.asarray(rays, f32).reshape(-1, 8)
    r = rays.astype(f64)
    ta, tb, _ = _clipped(surface, r)
    lines = _window(surface.X, r[:, 0], r[:, 4], ta, tb)[1] + _window(surface.Z, r[:, 2], r[:, 6], ta, tb)[1] + 2
    order = np.argsort(lines, kind="stable")
    parts, i = [], 0
    while i < len(order) or not parts:
        j = len(order)
        if j:  # (the counts ascend: the chunk's last ray sets its width)
            j = min(j, i + max(64, budget // int(lines[order[i]])))
            j = min(j, i + max(64, budget // int(lines[order[j - 1]])))
        parts.append(_terrain_chunk(surface, rays[order[i:j]], inv_two_r_prime, curved))
        i = max(j, i + 1)
    back = np.empty(len(order), np.int64)
    back[order] = np.arange(len(order))
    return {key: np.concatenate([p[key] for p in parts])[back] for key in parts[0]}


def lowest_before(surface, rays, t, inv_two_r_prime=0.0, curved=False):
    """(n,) minimum of f over [tmin, t] of each ray (+inf where that interval does not pass over the footprint)."""
    cut = np.asarray(rays, f32).copy()
    cut[:, 7] = np.asarray(t, f32)
    return terrain_reference(surface, cut, inv_two_r_prime, curved)["clear"]


def dense_trace(surface, ray, inv_two_r_prime=0.0, curved=False, samples_per_cell=2000):
    """Brute force for ONE ray: f on a dense parameter set over [tmin, tmax] clipped to the footprint.  Returns the bracket
    (t_before, t_at) of the first sample at which f <= 0 after a sample at which it was > 0 ((inf, inf) without one), the
    minimum of f over the samples, the largest step of f between neighbours (what a sample can miss) and whether the first
    sample is already <= 0.  None when the ray never passes over the footprint."""
    r = np.asarray(ray, f32).astype(f64)
    ox, oy, oz, tmin, dx, dy, dz, tmax = r
    k = (dx * dx + dz * dz) * f64(inv_two_r_prime) if curved else 0.0
    lo_x, hi_x = _axis_interval(surface.X, np.array([ox]), np.array([dx]))
    lo_z, hi_z = _axis_interval(surface.Z, np.array([oz]), np.array([dz]))
    ta, tb = max(tmin, lo_x[0], lo_z[0]), min(tmax, hi_x[0], hi_z[0])
    if not tb > ta:
        return None
    t = np.linspace(ta, tb, samples_per_cell * (surface.rows + surface.cols))
    f = oy + t * dy + k * t * t - surface.height(ox + t * dx, oz + t * dz)
    under = f <= 0.0
    change = np.nonzero(under[1:] & ~under[:-1])[0]
    bracket = (float(t[change[0]]), float(t[change[0] + 1])) if len(change) else (np.inf, np.inf)
    return {"bracket": bracket, "clear": float(f.min()), "step": float(np.abs(np.diff(f)).max()), "starts_under": bool(under[0]),
            "dt": float(t[1] - t[0])}


# ---- mesh ----------------------------------------------------------------------------------------------------------------
def triangle_search(vertices, indices, rays):
    """float64 Moeller-Trumbore of every ray (n, 8) against every triangle: t (n, M), inf where the reference shader's test
    refuses the pair, and the barycentric coordinates u, v and the determinant a (n, M) as computed (NaN where a == 0)."""
    r = np.asarray(rays, f32).astype(f64)
    verts, tris = np.asarray(vertices, f32).astype(f64), np.asarray(indices).reshape(-1, 3)
    o, d = r[:, None, 0:3], r[:, None, 4:7]
    v0, v1, v2 = (verts[tris[:, c]][None, :, :] for c in range(3))
    e1, e2 = v1 - v0, v2 - v0
    hh = np.cross(d, e2)
    a = (e1 * hh).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / a
        s = o - v0
        u = inv * (s * hh).sum(-1)
        q = np.cross(s, e1)
        v = inv * (d * q).sum(-1)
        t = inv * (e2 * q).sum(-1)
        ok = (np.abs(a) >= 1e-7) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > r[:, None, 3]) & (t < r[:, None, 7])
    return np.where(ok, t, np.inf), u, v, a


def mesh_reference(vertices, indices, rays):
    """Nearest triangle of each ray: `t` (n,) (inf: none), `triangle` (n,) (-1: none), and `margin` (n,): the smallest
    distance to a triangle's edge in barycentric units, |min(u, v, 1 - u - v)|, over the triangles whose plane the ray meets
    with t in range at a point inside the triangle or within MESH_NEAR of it (inf: none).  A small margin says the answer
    hangs on the rounding of an edge test."""
    t, u, v, a = triangle_search(vertices, indices, rays)
    r = np.asarray(rays, f32).astype(f64)
    verts, tris = np.asarray(vertices, f32).astype(f64), np.asarray(indices).reshape(-1, 3)
    p = verts[tris]
    longest = np.max([np.linalg.norm(p[:, i] - p[:, (i + 1) % 3], axis=1) for i in range(3)], axis=0)[None, :]
    with np.errstate(all="ignore"):
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        # the plane's own t, whatever the edge tests say
        o, d = r[:, None, 0:3], r[:, None, 4:7]
        e1, e2 = (p[:, 1] - p[:, 0])[None], (p[:, 2] - p[:, 0])[None]
        tt = (e2 * np.cross(o - p[None, :, 0], e1)).sum(-1) / a
        near = (np.abs(a) >= 1e-7) & (tt > r[:, None, 3]) & (tt < r[:, None, 7]) & ((m >= 0.0) | (-m * longest <= MESH_NEAR))
    margin = np.where(near, np.abs(m), np.inf).min(axis=1)
    nearest = np.argmin(t, axis=1)
    best = t[np.arange(len(t)), nearest]
    return {"t": best, "triangle": np.where(np.isfinite(best), nearest, -1), "margin": margin}
