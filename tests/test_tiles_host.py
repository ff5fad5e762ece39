"""The tile geometry of the frame path (csrc/f3d_tiles.h) on the host: ONE text says which pixels a wave's tile holds, how
many tiles a band has, how many workgroups a launch needs and which tile each of them renders -- the kernels (f3d_frame.h
tile_pixel / lane_pixel) and the launchers (f3d_kernels.hip frame_grid, frame_tile_count, launch_tile_order; f3d_host.hip
f3d_session_row_costs) all call it.  tests/tiles_host/tiles_harness.cpp checks the two halves of that contract against each
other, exhaustively over small shapes, and spreads tile costs over rows for the comparison below.  No GPU."""
from __future__ import annotations

import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from emul import emul

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "tiles_host" / "tiles_harness.cpp"
WIDTHS, ROWS, LANES = range(1, 34), range(0, 18), (1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def _program() -> Path:
    """The harness as a stand-alone program (its own main), with the emulator's flags."""
    out = Path(tempfile.mkdtemp(prefix="f3d_tiles_host_")) / "tiles_harness"
    flags = [f for f in emul.CXX if f not in ("-shared", "-fPIC")]
    subprocess.run([*flags, str(HARNESS), "-o", str(out)], check=True, capture_output=True)
    return out


def _run(*args, stdin=None):
    done = subprocess.run([str(_program()), *args], input=stdin, capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout


def test_every_launch_reaches_every_tile_once_and_the_tiles_every_pixel_of_the_band():
    """Width 1..33 x band rows 0..17 x band_begin {0, 5} x S {1, 2, 4, 8} x tile map {1, 2, 3}: tile_shape(lanes) is
    TileShape<S>; the tile count is tiles_x * tiles_y; the grid is 0 exactly when the band has no rows and a multiple of 8
    otherwise; workgroups [0, grid) reach tiles [0, ntiles) one-to-one and every other workgroup is padding; over all tiles
    and 64 lanes every pixel of the band is produced exactly S times, by S consecutive lanes, and every other produced pixel
    has gx >= width or gy >= band_end."""
    out = _run("check")
    assert int(re.search(r"check: (\d+) cases", out).group(1)) == 33 * 18 * 2 * 4 * 3, out


def _tile_counts(width, rows, lanes):
    """Tiles across and the tile height, as the row costs were written before the shared header."""
    log_s = {1: 0, 2: 1, 4: 2, 8: 3}[lanes]
    log_w = 3 if lanes <= 2 else 2
    log_h = 6 - log_s - log_w
    return (width + (1 << log_w) - 1) >> log_w, 1 << log_h


def _row_costs(cost, width, rows, lanes):
    """The row spreading in numpy, in the summation order of f3d_session_row_costs: double sums in ascending tile id, a
    tile's cost split over its rows (r1 - r0 of them: the last tile row may be ragged), one cast to float at the end."""
    tiles_x, th = _tile_counts(width, rows, lanes)
    sums = np.zeros(rows, np.float64)
    for t, c in enumerate(cost):
        r0 = (t // tiles_x) * th
        r1 = min(rows, r0 + th)
        sums[r0:r1] += np.float64(c) / np.float64(r1 - r0)
    return sums.astype(np.float32)


def test_tile_costs_spread_over_rows_are_the_numpy_sums_bit_for_bit():
    """Random integer tile costs (small ones, and the whole range of the 32-bit tick counters) on every width 1..33 x rows
    0..17 x S: the harness's floats are the bits of the numpy transcription, and add up to the costs.  The bound on the sum:
    a row value is a double sum rounded to float once, 2^-24 of its value at most; the double sums themselves are off by
    (tiles_x + 1) roundings of 2^-53 each, below 2^-40 of the costs on these shapes."""
    rng = np.random.default_rng(20240607)
    cases, lines = [], []
    for width in WIDTHS:
        for rows in ROWS:
            for lanes in LANES:
                tiles_x, th = _tile_counts(width, rows, lanes)
                tiles = tiles_x * ((rows + th - 1) // th)
                top = 1000 if (width + rows + lanes) % 2 else 2 ** 32
                cost = rng.integers(0, top, size=tiles, dtype=np.uint64).astype(np.uint32)
                cases.append((cost, width, rows, lanes))
                lines.append(" ".join(map(str, (width, rows, lanes, *cost.tolist()))))
    got_lines = _run("spread", stdin="\n".join(lines) + "\n").split("\n")[:-1]
    assert len(got_lines) == len(cases) == 33 * 18 * 4
    ragged = 0
    for (cost, width, rows, lanes), line in zip(cases, got_lines):
        got = np.array([int(word, 16) for word in line.split()], np.uint32).view(np.float32)
        want = _row_costs(cost, width, rows, lanes)
        assert got.shape == want.shape == (rows,), (width, rows, lanes)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (width, rows, lanes, got, want)
        total, rows_total = float(cost.astype(np.float64).sum()), float(got.astype(np.float64).sum())
        assert abs(rows_total - total) <= 2.0 ** -24 * rows_total + 2.0 ** -40 * total, (width, rows, lanes, rows_total, total)
        ragged += rows % _tile_counts(width, rows, lanes)[1] != 0
    assert ragged > 1000  # (most of the shapes end in a ragged tile row)
