"""The layouts of the paint's, the contours', the drainage's and the fill's scratch (csrc/f3d_scratch_carve.h), without a GPU.

tests/scratch_carve_host/scratch_carve.cpp -- a stand-alone program that includes that header alone -- prints, for every
family, every piece's offset and the total, the host form's outputs behind the pieces included; here they are compared with
the formulas each family carried when it laid its scratch out by hand (f3d_host_paint.h, f3d_host_contour.h,
f3d_host_drainage.h before the carver), with A(b) = b rounded up to 256:
    drainage         A(4 * 35 * 256) counters, A(n) code, 5 planes of A(4n); then A(n), A(4n), A(4n) of the region's planes
    fill             A(4 * 4 * 256) counters, 2 planes of A(4 * tiles) flags, 3 planes of A(4n); then 3 x A(4n)
    filled drainage  the drainage's pieces, the fill's behind them, then the drainage's outputs
    streams          behind the drainage's pieces: 2 x A(8 * (waves + 1)), A(scan); then A(16 r), A(4 r) of the records
    contours         2 x A(8 * (blocks + 1)), A(4 * levels), A(scan); then A(16 r), A(4 r)
    paint records    A(80 r), 2 x A(8 * (r + 1)), 256 for the run counter, A(scan)
    paint keys       2 x A(8 k), A(4 * min(k, tiles)), A(sort)
over DEMs of 2x2, 9x9, 64x64, 65x63 and 2049x2049 samples, 1, 2 and 4 tiles, 1, 2 and 65 waves or blocks, 1, 64 and 65
levels, 0, 1, 3, 16 and 17 records, every subset of a family's outputs, and 0, 1 and 4096 bytes of scan storage (on the
device rocPRIM names that figure).  The fill's pieces lie at the same offsets from their base alone and behind the routing's
pieces.  The same program built with -fsanitize=address,undefined runs clean.
The sizes a live session reports after such calls: tests/test_gpu_derived_shared.py.
"""
from __future__ import annotations

import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "scratch_carve_host" / "scratch_carve.cpp"
SAMPLES = (2 * 2, 9 * 9, 64 * 64, 65 * 63, 2049 * 2049)
TILES, GROUPS, LEVELS, RECORDS, SCANS = (1, 2, 4), (1, 2, 65), (1, 64, 65), (0, 1, 3, 16, 17), (0, 1, 4096)
DRAIN_COUNTERS, FILL_COUNTERS = 35 * 256, 4 * 256  # words: (3 + 32 rounds) x 256 slots, 4 x 256 slots


def A(b):
    return (b + 255) & ~255


def behind(base, subset, sizes):
    """Offsets of the outputs of ``subset`` behind ``base``, each rounded to 256, an absent one 0 bytes; the total."""
    at = []
    for k, b in enumerate(sizes):
        at.append(base)
        base += A(b) if subset >> k & 1 else 0
    return at, base


def drainage_pieces(n):
    planes = A(4 * DRAIN_COUNTERS) + A(n)
    return [0, A(4 * DRAIN_COUNTERS)] + [planes + k * A(4 * n) for k in range(5)], planes + 5 * A(4 * n)


def fill_pieces(n, tiles, base=0):
    flags, planes = base + A(4 * FILL_COUNTERS), base + A(4 * FILL_COUNTERS) + 2 * A(4 * tiles)
    return [base, flags, flags + A(4 * tiles), planes, planes + A(4 * n), planes + 2 * A(4 * n)], planes + 3 * A(4 * n)


def drainage(n, subset, scan):
    pieces, fixed = drainage_pieces(n)
    assert fixed == A(4 * DRAIN_COUNTERS) + A(n) + 5 * A(4 * n)
    out, total = behind(fixed, subset, (n, 4 * n, 4 * n))
    return pieces + out, total


def fill(n, tiles, subset, scan):
    pieces, fixed = fill_pieces(n, tiles)
    assert fixed == A(4 * FILL_COUNTERS) + 2 * A(4 * tiles) + 3 * A(4 * n)
    out, total = behind(fixed, subset, (4 * n, 4 * n, 4 * n))
    return pieces + out, total


def filled_drainage(n, tiles, subset, scan):
    pieces, unfilled = drainage_pieces(n)
    more, fixed = fill_pieces(n, tiles, unfilled)
    assert fixed == A(4 * DRAIN_COUNTERS) + A(n) + 5 * A(4 * n) + A(4 * FILL_COUNTERS) + 2 * A(4 * tiles) + 3 * A(4 * n)
    out, total = behind(fixed, subset, (n, 4 * n, 4 * n))
    return pieces + more + out + [unfilled], total


def streams(n, waves, r, subset, scan):
    routed, words = drainage_pieces(n)[1], A(8 * (waves + 1))
    out, total = behind(routed + 2 * words + A(scan), subset, (16 * r, 4 * r))
    return [routed, routed + words, routed + 2 * words] + out, total


def contours(blocks, levels, r, subset, scan):
    words = A(8 * (blocks + 1))
    out, total = behind(2 * words + A(4 * levels) + A(scan), subset, (16 * r, 4 * r))
    return [0, words, 2 * words, 2 * words + A(4 * levels)] + out, total


def paint_records(r, scan):
    rec, words = A(80 * r), A(8 * (r + 1))
    return [0, rec, rec + words, rec + 2 * words, rec + 2 * words + 256], rec + 2 * words + 256 + A(scan)


def paint_keys(k, tiles, scan):
    keys, runs = A(8 * k), A(4 * min(k, tiles))
    return [0, keys, 2 * keys, 2 * keys + runs], 2 * keys + runs + A(scan)


FORMULAS = {"drainage": drainage, "fill": fill, "filled-drainage": filled_drainage, "streams": streams, "contours": contours,
            "paint-records": paint_records, "paint-keys": paint_keys}


def build(*flags):
    out = Path(tempfile.mkdtemp(prefix="f3d_scratch_carve_")) / "scratch_carve"
    made = subprocess.run(["g++", "-std=c++17", *flags, str(SOURCE), "-o", str(out)], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-2000:]
    return out


def table():
    want = {("drainage", n, s) for n in SAMPLES for s in range(8)}
    want |= {(f, n, t, s) for f in ("fill", "filled-drainage") for n in SAMPLES for t in TILES for s in range(8)}
    want |= {("streams", n, w, r, s) for n in SAMPLES for w in GROUPS for r in RECORDS for s in range(4)}
    want |= {("contours", b, lv, r, s) for b in GROUPS for lv in LEVELS for r in RECORDS for s in range(4)}
    want |= {("paint-records", r) for r in RECORDS} | {("paint-keys", r, t) for r in RECORDS for t in TILES}
    return want


@pytest.fixture(scope="module")
def program():
    return build("-O2")


@pytest.mark.parametrize("scan", SCANS)
def test_layouts_equal_the_formulas_the_families_carried(program, scan):
    run = subprocess.run([str(program), str(scan)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    seen, alone = set(), {}
    for line in run.stdout.splitlines():
        head, offsets, total = line.split("|")
        family, *counts = head.split()
        case = (family, *(int(v) for v in counts))
        got = [int(v) for v in offsets.split()]
        want_offsets, want_total = FORMULAS[family](*case[1:], scan)
        assert got == want_offsets and int(total) == want_total, (case, line)
        assert all(v % 256 == 0 for v in got) and int(total) % 256 == 0, "every piece starts on a multiple of 256"
        assert case not in seen
        seen.add(case)
        # the fill's six pieces from their base: alone (f3d_session_fill) and behind the routing's (drain_route)
        if family == "fill":
            alone[case[1:]] = got[:6]
        if family == "filled-drainage":
            assert [v - got[-1] for v in got[7:13]] == alone[case[1:]], ("the fill's layout is one, wherever it is placed", case)
    assert seen == table(), "every case of the table, once"
    # the figures the ABI header states a sample: 21 bytes routed, 33 over the filled surface, 12 for the fill alone
    n = 2049 * 2049
    assert drainage(n, 0, 0)[1] // n == 21 and filled_drainage(n, 4, 0, 0)[1] // n == 33 and fill(n, 4, 0, 0)[1] // n == 12


def test_program_runs_clean_under_address_and_undefined_sanitizers():
    out = build("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    run = subprocess.run([str(out), "4096"], capture_output=True, text=True, env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert len(run.stdout.splitlines()) == len(table()) and "ERROR" not in run.stderr and "runtime error" not in run.stderr
