#!/usr/bin/env python
"""The bits the raster lane bodies (horizon, clearance, umbra walks; the five families' lattice points) return at a given
commit, for tests/test_walk_bits_host.py and tests/test_gpu_walk_bits.py: tests/golden/raster_walk_bits.npz.

    git worktree add --detach /tmp/f3d_parent <commit>
    python tests/golden/make_walk_bits.py /tmp/f3d_parent

Builds the host harnesses OF THAT CHECKOUT (tests/*_host/*.cpp over its forge3d_amd/csrc) with emul.CXX and runs the cases of
tests/walk_bits.py.  The fixture holds the inputs, the checkout's commit hash, the SHA-256 of every output plane's
little-endian f32 bytes (one for both wave footprints: they must agree), and the planes themselves, end to end, for the DEMs
of at most 18 samples.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]

import walk_bits as wb  # noqa: E402


def main(checkout):
    commit = subprocess.run(["git", "-C", checkout, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    harnesses = wb.build_harnesses(Path(checkout))
    out = {k: v for k, v in wb.make_inputs(harnesses).items()}
    keys, digests, plane_keys, planes, nans = [], [], [], [], 0
    for shape in wb.SHAPES:
        seen = {}
        for key, plane in wb.host_cases(harnesses, out, shape):
            d = wb.digest(plane)
            if "/cap/" not in key:
                nans += int(np.isnan(plane).sum())
            if key != wb.stored_key(key):  # the two wave footprints own the same samples: one digest serves both
                assert seen[wb.stored_key(key)] == d, f"{key}: the footprints differ"
                continue
            seen[key] = d
            keys.append(key)
            digests.append(np.frombuffer(bytes.fromhex(d), np.uint8))
            if shape[0] * shape[1] <= wb.FULL_PLANES_UP_TO:
                plane_keys.append(key)
                planes.append(np.ascontiguousarray(plane, "<f4").ravel())
    assert nans == 0, "a walk without an injected cap reached it"
    out["keys"], out["digests"], out["commit"] = np.array(keys), np.stack(digests), np.array(commit)
    out["plane_keys"], out["planes"] = np.array(plane_keys), np.concatenate(planes)
    out["plane_starts"] = np.concatenate([[0], np.cumsum([len(p) for p in planes])]).astype(np.int64)
    path = HERE / "raster_walk_bits.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {len(keys)} planes at {commit}, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
