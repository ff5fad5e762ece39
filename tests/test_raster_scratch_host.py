"""The layout of the rasters' host-form scratch (csrc/f3d_raster_scratch.h: scratch_layout), without a GPU.

tests/raster_scratch_host/raster_scratch.cpp -- a stand-alone program that includes that header alone -- prints, for the
segment lists of the four families (csrc/f3d_host_rasters.h), every segment's offset and the total; here they are compared
with the formulas each family carried when it laid its scratch out by itself:
    raster       masks, round up to 16, targets, count
    horizon      planes, sky_view, round up to 16, azimuths (8 bytes each)
    irradiation  energy, count, normals, round up to 16, directions
    clearance    planes, lowest, round up to 16, observers
over n in {1, 3, 63 * 65, 2049 * 2049} samples, K in {0, 1, 3, 16, 256} inputs, every subset of a family's outputs, and the
raster without an input (SESSION_SUN).  The same program built with -fsanitize=address,undefined runs clean.
The sizes a live session reports after such calls: tests/test_gpu_rasters_shared.py and the families' own GPU suites.
"""
from __future__ import annotations

import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "raster_scratch_host" / "raster_scratch.cpp"
SAMPLES = (1, 3, 63 * 65, 2049 * 2049)
INPUTS = (0, 1, 3, 16, 256)


def room(b):
    return (b + 15) & ~15


def raster(n, k, subset, sun):
    masks, count = subset & 1, subset >> 1 & 1
    k = 1 if sun else k
    mask_bytes, target_bytes, count_bytes = (k * ((n + 63) // 64) * 8 if masks else 0), (0 if sun else k * 16), (n * 4 if count else 0)
    return [0, room(mask_bytes), room(mask_bytes) + target_bytes], room(mask_bytes) + target_bytes + count_bytes


def planes_then_one(row_bytes):
    def family(n, k, subset, sun):
        plane_bytes, one_bytes = (k * n * 4 if subset & 1 else 0), (n * 4 if subset >> 1 & 1 else 0)
        return [0, plane_bytes, room(plane_bytes + one_bytes)], room(plane_bytes + one_bytes) + k * row_bytes
    return family


def irradiation(n, k, subset, sun):
    energy, count, normal = (n * 4 if subset & 1 else 0), (n * 4 if subset >> 1 & 1 else 0), (n * 12 if subset >> 2 & 1 else 0)
    return [0, energy, energy + count, room(energy + count + normal)], room(energy + count + normal) + k * 16


FORMULAS = {"raster": raster, "horizon": planes_then_one(8), "clearance": planes_then_one(16), "irradiation": irradiation}


def build(*flags):
    out = Path(tempfile.mkdtemp(prefix="f3d_raster_scratch_")) / "raster_scratch"
    made = subprocess.run(["g++", "-std=c++17", *flags, str(SOURCE), "-o", str(out)], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-2000:]
    return out


def test_layouts_equal_the_four_formulas():
    run = subprocess.run([str(build("-O2"))], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    seen = set()
    for line in run.stdout.splitlines():
        head, offsets, total = line.split("|")
        family, n, k, subset, sun = head.split()
        case = (family, int(n), int(k), int(subset), int(sun))
        want_offsets, want_total = FORMULAS[family](*case[1:])
        assert [int(v) for v in offsets.split()] == want_offsets and int(total) == want_total, (case, line)
        seen.add(case)
    want = {(f, n, k, subset, sun) for f in FORMULAS for n in SAMPLES for k in INPUTS for subset in range(8 if f == "irradiation" else 4)
            for sun in ((0, 1) if f == "raster" else (0,))}
    assert seen == want, "every case of the table, once"
    # the sizes where the rounding shows (tests/test_gpu_rasters_shared.py asks a live session for them)
    assert FORMULAS["horizon"](1, 1, 3, 0)[1] == 24 and FORMULAS["clearance"](1, 1, 3, 0)[1] == 32
    assert raster(1, 1, 3, 0)[1] == 36 and irradiation(1, 1, 7, 0)[1] == 48


def test_program_runs_clean_under_address_and_undefined_sanitizers():
    out = build("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    run = subprocess.run([str(out)], capture_output=True, text=True, env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert len(run.stdout.splitlines()) == 4 * 5 * (2 * 4 + 4 + 4 + 8) and "ERROR" not in run.stderr and "runtime error" not in run.stderr
