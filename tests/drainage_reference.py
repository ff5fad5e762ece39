"""An independent statement of the drainage contract (csrc/f3d_drainage.h) -- TEST INFRASTRUCTURE ONLY.

NumPy, sample by sample; it knows nothing of waves, tiles or path doubling:
* directions: a loop over the eight neighbours in float32 (slopes(), and their float64 twin);
* accumulation: the samples visited in descending height, each handing its count to its receiver;
* basins: the receivers followed to their sink;
* streams: a row-major filter over the region's samples.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
SINK = 8
# (d_row, d_col) of codes 0 .. 7: E, SE, S, SW, W, NW, N, NE -- +col east, +row south
STEPS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))


def session_heights(dem, exaggeration):
    """The heights a session holds: f32(h * exaggeration)."""
    return (np.asarray(dem, f32) * f32(exaggeration)).astype(f32)


def runs(spacing, dtype=f32):
    """The eight runs: spacing_x for E/W, spacing_z for N/S, the diagonal -- two products, one sum, one sqrt, each rounded to
    `dtype` -- for the rest."""
    sx, sz = dtype(spacing[0]), dtype(spacing[1])
    diag = np.sqrt(dtype(dtype(sx * sx) + dtype(sz * sz)))
    return [dtype(diag) if k & 1 else (sz if k & 2 else sx) for k in range(8)]


def slopes(heights, spacing, dtype=f32):
    """(8, H, W) of `dtype`: (h - h_neighbour) / run per code, NaN where the neighbour does not exist."""
    h = np.asarray(heights, f32).astype(dtype)
    rows, cols = h.shape
    out = np.full((8, rows, cols), np.nan, dtype)
    run = runs(spacing, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (dj, di) in enumerate(STEPS):
            for j in range(max(0, -dj), min(rows, rows - dj)):
                i0, i1 = max(0, -di), min(cols, cols - di)
                out[k, j, i0:i1] = ((h[j, i0:i1] - h[j + dj, i0 + di:i1 + di]).astype(dtype) / run[k]).astype(dtype)
    return out


def directions(heights, spacing):
    """uint8 (H, W): the code with the largest float32 slope > 0, the lowest code of equals; SINK without one."""
    s = slopes(heights, spacing)
    rows, cols = s.shape[1:]
    code = np.full((rows, cols), SINK, np.uint8)
    for j in range(rows):
        for i in range(cols):
            best = f32(0.0)
            for k in range(8):
                v = s[k, j, i]
                if v > best:  # (NaN compares false)
                    best, code[j, i] = v, k
    return code


def receivers(code):
    """int64 (H * W,): the linear index of each sample's receiver; a sink's own."""
    rows, cols = code.shape
    j, i = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    dj = np.array([s[0] for s in STEPS] + [0])[code]
    di = np.array([s[1] for s in STEPS] + [0])[code]
    return ((j + dj) * cols + (i + di)).reshape(-1).astype(np.int64)


def route(heights, spacing):
    """{"direction" uint8 (H, W), "accumulation" uint32 (H, W), "basin" uint32 (H, W), "sinks", "longest"} of the whole DEM."""
    h = np.asarray(heights, f32)
    code = directions(h, spacing)
    recv = receivers(code)
    n = h.size
    flat = h.reshape(-1)
    sink = code.reshape(-1) == SINK
    assert (flat[recv[~sink]] < flat[~sink]).all(), "a receiver is strictly lower"
    acc = np.ones(n, np.int64)
    # descending height: every sample comes before its receiver.  (A NaN height is a sink nobody drains into: its place in
    # the order does not matter.)
    order = np.argsort(-np.where(np.isnan(flat), -np.inf, flat.astype(np.float64)), kind="stable")
    for v in order:
        if not sink[v]:
            acc[recv[v]] += acc[v]
    basin = np.full(n, -1, np.int64)
    depth = np.zeros(n, np.int64)
    for v in order[::-1]:  # ascending: a receiver before those that drain into it
        basin[v] = v if sink[v] else basin[recv[v]]
        depth[v] = 0 if sink[v] else depth[recv[v]] + 1
    assert (basin >= 0).all()
    return {"direction": code, "accumulation": acc.astype(np.uint32).reshape(h.shape), "basin": basin.astype(np.uint32).reshape(h.shape),
            "sinks": int(sink.sum()), "longest": int(depth.max())}


def rounds(longest):
    """floor(log2(longest)) + 1 doubling rounds have a live sample; none on a flat."""
    return 0 if longest == 0 else int(longest).bit_length()


def plane_at(origin, index, spacing):
    """f32 fma(index, spacing, origin): the lattice's own coordinate, rounded once (float64 holds the product and sum of
    float32 values of this size exactly enough: 24 + 24 bits of product, one rounding to float32)."""
    return (np.asarray(index, np.float64) * np.float64(f32(spacing)) + np.float64(f32(origin))).astype(f32)


def streams(routed, origin, spacing, threshold, region=None):
    """{"segments" (N, 4) float32, "accumulation" (N,) uint32, "sample" (N,) linear indices}: row-major over the region."""
    code, acc = routed["direction"], routed["accumulation"]
    rows, cols = code.shape
    row0, col0, nr, nc = (0, 0, rows, cols) if region is None else region
    seg, out_acc, sample = [], [], []
    for j in range(row0, row0 + nr):
        for i in range(col0, col0 + nc):
            k = int(code[j, i])
            if k == SINK or acc[j, i] < threshold:
                continue
            dj, di = STEPS[k]
            seg.append([plane_at(origin[0], i, spacing[0]), plane_at(origin[1], j, spacing[1]),
                        plane_at(origin[0], i + di, spacing[0]), plane_at(origin[1], j + dj, spacing[1])])
            out_acc.append(acc[j, i])
            sample.append(j * cols + i)
    return {"segments": np.array(seg, f32).reshape(-1, 4), "accumulation": np.array(out_acc, np.uint32), "sample": np.array(sample, np.int64)}
