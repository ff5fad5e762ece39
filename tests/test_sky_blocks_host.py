"""The deep-sky block rule (csrc/f3d_skyblocks.h) on the host: ONE text says which 8 x 8 blocks of a strip are deep -- every
pixel of the block's rectangle [x0 - 4, x0 + 12) x [y0 - 4, y0 + 12) holds the sky certificate, pixels outside the image
counting as certified and rows of another strip as not -- and which block a frame-kernel tile lies in.  k_sky_blocks, k_head,
frame_wave and f3d_session_sky_blocks call it; tests/sky_blocks_host/sky_blocks_harness.cpp runs it lane by lane against
the NumPy erosion below, exhaustively over small shapes.  No GPU."""
from __future__ import annotations

import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from emul import emul

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "sky_blocks_host" / "sky_blocks_harness.cpp"
MARGIN = 4


def _build(*extra) -> Path:
    out = Path(tempfile.mkdtemp(prefix="f3d_sky_blocks_host_")) / "sky_blocks_harness"
    flags = [f for f in emul.CXX if f not in ("-shared", "-fPIC")]
    if extra:
        flags = [f for f in flags if f != "-O2"]
    done = subprocess.run([*flags, *extra, str(HARNESS), "-o", str(out)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    return out


@functools.lru_cache(maxsize=None)
def _program() -> Path:
    """The harness as a stand-alone program (its own main), with the emulator's flags."""
    return _build()


def _deep_reference(mask, height, row_begin):
    """The rectangle rule as an erosion: the owned rows' certificates in the image, False in the rows of other strips, True
    around the image; a block is deep when its 16 x 16 window holds no False."""
    rows, width = mask.shape
    image = np.zeros((height, width), bool)
    image[row_begin:row_begin + rows] = mask
    blocks_x, blocks_y = (width + 7) // 8, (rows + 7) // 8
    padded = np.ones((MARGIN + row_begin + blocks_y * 8 + MARGIN + height, MARGIN + blocks_x * 8 + MARGIN), bool)
    padded[MARGIN:MARGIN + height, MARGIN:MARGIN + width] = image
    windows = np.lib.stride_tricks.sliding_window_view(padded, (16, 16))[row_begin::8, ::8][:blocks_y, :blocks_x]
    return windows.all(axis=(2, 3))


def _classify(cases, program=None):
    """cases: (mask of the owned rows, image height, row_begin) each -> the harness's deep flags, (blocks_y, blocks_x) each."""
    text = []
    for mask, height, row_begin in cases:
        rows, width = mask.shape
        text.append(f"{width} {height} {row_begin} {row_begin + rows} " + "".join("1" if v else "0" for v in mask.ravel()))
    done = subprocess.run([str(program or _program()), "classify"], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-500:], done.stderr[-3000:])
    assert "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-3000:]
    lines = done.stdout.split()
    assert len(lines) == len(cases), (len(lines), len(cases))
    out = []
    for line, (mask, _, _) in zip(lines, cases):
        rows, width = mask.shape
        out.append((np.frombuffer(line.encode(), np.uint8) == ord("1")).reshape((rows + 7) // 8, (width + 7) // 8))
    return out


def _check(cases, program=None):
    deep_blocks = 0
    for got, (mask, height, row_begin) in zip(_classify(cases, program), cases):
        want = _deep_reference(mask, height, row_begin)
        assert np.array_equal(got, want), (mask.shape, height, row_begin, np.argwhere(got != want)[:4])
        deep_blocks += int(want.sum())
    return deep_blocks


def _small_cases():
    """Widths and heights 1 ... 40, the strip the whole image: all certified, and a random mask dense enough to leave deep
    blocks beside shallow ones."""
    rng = np.random.default_rng(20261019)
    cases = []
    for width in range(1, 41):
        for height in range(1, 41):
            cases.append((np.ones((height, width), bool), height, 0))
            cases.append((rng.random((height, width)) < 0.995, height, 0))
    return cases


def test_deep_is_the_rectangle_rule_over_every_small_shape():
    cases = _small_cases()
    deep = _check(cases)
    # (not vacuous: an all-certified whole image is all deep, and the random masks leave both kinds)
    all_deep = sum(((h + 7) // 8) * ((w + 7) // 8) for w in range(1, 41) for h in range(1, 41))
    assert all_deep < deep < 2 * all_deep, (deep, all_deep)


def test_owned_row_ranges_inside_a_taller_image():
    """A strip knows nothing of its neighbours' certificates: the rows of another strip count as not certified, the rows
    outside the image as certified -- so with every owned pixel certified a block is deep exactly when its rectangle's rows
    inside the image are all owned."""
    rng = np.random.default_rng(7)
    cases, geometry = [], []
    for height in (24, 33, 40):
        for row_begin, row_end in ((0, height), (5, 29), (8, 24), (3, height), (0, 17), (13, 14), (4, 20), (height - 9, height)):
            if not 0 <= row_begin < row_end <= height:
                continue
            for width in (1, 7, 8, 9, 16, 23, 40):
                rows = row_end - row_begin
                cases.append((np.ones((rows, width), bool), height, row_begin))
                cases.append((rng.random((rows, width)) < 0.99, height, row_begin))
                geometry.append((height, row_begin, row_end, width))
    assert _check(cases) > 0
    for got, (height, row_begin, row_end, width) in zip(_classify(cases[0::2]), geometry):
        for by in range(got.shape[0]):
            y0 = row_begin + 8 * by
            owned = max(y0 - MARGIN, 0) >= row_begin and min(y0 + 8 + MARGIN, height) <= row_end
            assert bool(got[by].all()) == owned and bool(got[by].any()) == owned, (height, row_begin, row_end, width, by)


def test_a_single_uncertified_pixel_at_every_distance_from_a_block():
    """One pixel without the certificate at Chebyshev distance 0 ... 5 from block (2, 2) of a 40 x 40 image, on every side
    and corner: the block is deep only at distance 5; distance 0 is a pixel of the block itself."""
    x0 = y0 = 16
    cases, distances = [], []
    for d in range(0, 6):
        lo, hi = x0 - d, x0 + 7 + d
        spots = {(lo, lo), (lo, hi), (hi, lo), (hi, hi), (lo, y0 + 3), (hi, y0 + 4), (x0 + 3, lo), (x0 + 4, hi)}
        for x, y in sorted(spots):
            mask = np.ones((40, 40), bool)
            mask[y, x] = False
            cases.append((mask, 40, 0))
            distances.append(d)
    _check(cases)
    for got, d in zip(_classify(cases), distances):
        assert bool(got[2, 2]) == (d == 5), d
        assert got.sum() >= 25 - 9  # the pixel reaches the blocks around it at most


def test_every_frame_tile_lies_in_exactly_one_block():
    done = subprocess.run([str(_program()), "nest"], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout[-1000:], done.stderr[-2000:])
    assert int(re.search(r"nest: (\d+) cases", done.stdout).group(1)) == 40 * 40 * 4


def test_harness_runs_clean_under_address_and_undefined_sanitizers():
    """The same stand-alone program built with the sanitizers, over the tile nesting and a classification that reaches every
    clipping case: ragged widths, blocks on every rim, strips inside a taller image."""
    program = _build("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    env = {"ASAN_OPTIONS": "detect_leaks=1"}
    done = subprocess.run([str(program), "nest"], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-3000:]
    rng = np.random.default_rng(3)
    cases = [(rng.random((re_ - rb, w)) < 0.99, h, rb) for w in (1, 9, 33, 40) for h in (7, 40)
             for rb, re_ in ((0, h), (1, h - 1), (h // 2, h)) if rb < re_]
    assert _check(cases, program) >= 0
