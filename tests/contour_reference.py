"""An independent float64 statement of the contour contract (csrc/f3d_contour.h) -- TEST INFRASTRUCTURE ONLY.

Marching squares over cells: it knows nothing of blocks, bands, waves or scans.  Heights are the session's float32 heights
(f32(h * exaggeration)) taken to float64, so ``h >= level`` is the comparison the float32 body makes; positions are computed in
float64 from the float32 origin and spacing.  The output is in CELL order -- cells row-major over the region, levels ascending
in a cell, a case's segments in table order; ``block_order`` is the contract's reordering of it, stated on its own.
"""
from __future__ import annotations

import numpy as np

# a cell's lattice edges: B bottom (h00-h10, row j), R right (h10-h11, column i + 1), T top (h01-h11, row j + 1), L left
# (h00-h01, column i); per case the segments, each from its first crossing to its second
TABLE = {
    1: [("L", "B")], 2: [("B", "R")], 3: [("L", "R")], 4: [("T", "L")], 5: [("T", "B")], 6: [("B", "R"), ("T", "L")], 7: [("T", "R")],
    8: [("R", "T")], 9: [("L", "B"), ("R", "T")], 10: [("B", "T")], 11: [("L", "T")], 12: [("R", "L")], 13: [("R", "B")], 14: [("B", "L")],
}


def session_heights(dem, exaggeration):
    """The heights a session holds: f32(h * exaggeration), one float32 product."""
    return np.asarray(dem, np.float32) * np.float32(exaggeration)


def _crossing(edge, h00, h10, h01, h11, level, x0, z0, dx, dz):
    """(x, z) float64 of the crossings of `level` (an array of levels) on `edge` of the cell whose lower lattice point is (x0, z0)."""
    one = np.ones_like(level)
    if edge == "B":
        return x0 + (level - h00) / (h10 - h00) * dx, z0 * one
    if edge == "T":
        return x0 + (level - h01) / (h11 - h01) * dx, (z0 + dz) * one
    if edge == "L":
        return x0 * one, z0 + (level - h00) / (h01 - h00) * dz
    return (x0 + dx) * one, z0 + (level - h10) / (h11 - h10) * dz


def contours(heights32, origin, spacing, levels, region=None):
    """All segments of `region` (cells: row0, col0, rows, cols; None: all) in CELL order.  Returns a dict of arrays: ``cell``
    (cz * cell_w + cx), ``level_index``, ``case``, ``segment`` (0 or 1 within the case), ``xz`` (N, 4) float64."""
    h = np.asarray(heights32, np.float32).astype(np.float64)
    cell_h, cell_w = h.shape[0] - 1, h.shape[1] - 1
    row0, col0, rows, cols = (0, 0, cell_h, cell_w) if region is None else region
    ox, oz, dx, dz = float(np.float32(origin[0])), float(np.float32(origin[1])), float(np.float32(spacing[0])), float(np.float32(spacing[1]))
    lv = np.asarray(levels, np.float32).astype(np.float64)
    parts = []
    for j in range(row0, row0 + rows):
        for i in range(col0, col0 + cols):
            h00, h10, h01, h11 = h[j, i], h[j, i + 1], h[j + 1, i], h[j + 1, i + 1]
            case = (h00 >= lv) * 1 + (h10 >= lv) * 2 + (h01 >= lv) * 4 + (h11 >= lv) * 8
            ks = np.nonzero((case != 0) & (case != 15))[0]
            if ks.size == 0:
                continue
            x0, z0 = ox + i * dx, oz + j * dz
            for c in np.unique(case[ks]):
                kc = ks[case[ks] == c]
                for s, (ea, eb) in enumerate(TABLE[int(c)]):
                    ax, az = _crossing(ea, h00, h10, h01, h11, lv[kc], x0, z0, dx, dz)
                    bx, bz = _crossing(eb, h00, h10, h01, h11, lv[kc], x0, z0, dx, dz)
                    n = kc.size
                    parts.append((np.full(n, j * cell_w + i), kc, np.full(n, int(c)), np.full(n, s), np.stack([ax, az, bx, bz], 1)))
    if not parts:
        return {"cell": np.zeros(0, np.int64), "level_index": np.zeros(0, np.int64), "case": np.zeros(0, np.int64), "segment": np.zeros(0, np.int64),
                "xz": np.zeros((0, 4))}
    cell, lev, case, seg, xz = (np.concatenate([p[q] for p in parts]) for q in range(5))
    order = np.lexsort((seg, lev, cell))
    return {"cell": cell[order], "level_index": lev[order], "case": case[order], "segment": seg[order], "xz": xz[order]}


def block_order(got, cell_w):
    """The contract's order of a cell-ordered result: 8 x 8 blocks aligned to the cell grid row-major, then as it was."""
    cz, cx = got["cell"] // cell_w, got["cell"] % cell_w
    order = np.lexsort((np.arange(len(cz)), cx // 8, cz // 8))  # stable: cells row-major inside a block keep their order
    # (cells row-major over the region restricted to one block ARE row-major inside the block)
    return {k: v[order] for k, v in got.items()}


def polyline_length(points):
    p = np.asarray(points, np.float64)
    return float(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(1)).sum())
