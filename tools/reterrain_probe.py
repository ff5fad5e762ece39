"""What new heights cost a live session, against a new session: one GPU, one run, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM) at --width x --height (default 1920x1080), per mode --repeats
times, the device idle before every timed call:
  create      TerrainSession(...) on a DEM the scene cache does not hold (every repeat another DEM): what a frame of a
              time-lapse pays without the re-terrain -- host time of the call, its phases (setup_ms()), and the device
              time from the call's start to the end of its last pass (events on the session's stream);
  whole       TerrainSession.reterrain of the whole DEM;
  patch256    ... of a 256x256 patch;
  patch16     ... of a 16x16 patch.
For the re-terrains the host time is the asynchronous call alone and the device time runs from the call's start to the
end of the re-aim pass that closes it (staged upload, the two table kernels, k_reaim).  `upload_bytes` is what each
mode sends to the device.

    python tools/reterrain_probe.py [--dem 2048] [--width 1920] [--height 1080] [--repeats 7]

Launch counts: run the tool once, with nothing else in the run, under
`rocprofv3 --kernel-trace --stats -d DIR -o probe -- python tools/reterrain_probe.py --repeats 3 [--dem 64]`, then
    python tools/reterrain_probe.py --trace-db DIR --repeats 3
prints the kernels of the run and the launches per call (one JSON line).  The table kernels of a re-terrain are two
whatever the DEM's size.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODES = ("whole", "patch256", "patch16")


def trace_summary(root: str, repeats: int) -> dict:
    """Kernel launches of a rocprofv3 --kernel-trace database under `root`, by name; the re-terrain's per call."""
    import sqlite3

    dbs = sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 database under {root}")
    cur = sqlite3.connect(dbs[0]).cursor()
    rows = cur.execute("select name, count(*), sum(end-start) from kernels group by name").fetchall()
    out = {"database": os.path.relpath(dbs[0], root), "kernels": {}}
    for name, calls, total in sorted(rows):
        short = name.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
        rec = out["kernels"].setdefault(short, {"calls": 0, "total_ms": 0.0})
        rec["calls"] += calls
        rec["total_ms"] += total / 1e6
    calls = len(MODES) * repeats + 1  # (+ the one that gives the session its own tables)
    for label in ("k_retable_tiles", "k_retable_top", "k_reaim"):
        n = sum(v["calls"] for k, v in out["kernels"].items() if label in k)
        out[f"{label}_per_reterrain"] = n / calls
    builders = sum(v["calls"] for k, v in out["kernels"].items() if any(b in k for b in ("k_leaf_build", "k_level_build", "k_band_build")))
    # (creates that build tables: the warm-up, one per repeat, and the live session's -- its DEM has left the two-entry cache by then)
    out["table_build_launches_per_create"] = builders / (repeats + 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace-db", default=None, help="summarise a rocprofv3 --kernel-trace database directory instead")
    args = ap.parse_args()
    if args.trace_db:
        print(json.dumps(trace_summary(args.trace_db, args.repeats)))
        return

    import torch

    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, variance_threshold=1e30, max_frames=4, min_frames=4)
    W, H = args.width, args.height
    n = dem.shape[0]
    rng = np.random.default_rng(3)

    def timed(call):
        """(host ms of the call, device ms from its start to the end of what it enqueued)"""
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        result = call()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        torch.cuda.synchronize()
        return host, e0.elapsed_time(e1), result

    def stats(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    out = {"config": f"rainier proxy {n}^2, {W}x{H}, {args.repeats} repeats, device idle before every call"}
    # (1) the parent's way: a new session on a DEM the cache does not hold
    with TerrainSession(dem, W, H, cam, **kw):  # (warm-up: the runtime's and the library's first-use costs)
        pass
    host, device, phases = [], [], []
    for r in range(args.repeats):
        fresh = (dem + np.float32(0.25 * (r + 1))).astype(np.float32)
        h, d, s = timed(lambda: TerrainSession(fresh, W, H, cam, **kw))
        host.append(h), device.append(d), phases.append(s.setup_ms())
        s.close()
    out["create"] = {"host_ms": stats(host), "device_ms": stats(device), "upload_bytes": int(dem.nbytes),
                     "setup_ms_median": {k: statistics.median(p[k] for p in phases) for k in phases[0]}}
    # (2), (3) re-terrains of one live session
    side = {"whole": n, "patch256": min(256, n), "patch16": min(16, n)}
    with TerrainSession(dem, W, H, cam, **kw) as s:
        first = timed(lambda: s.reterrain(dem))
        out["first_reterrain"] = {"host_ms": first[0], "device_ms": first[1], "note": "takes the session's own tables and the staging buffer"}
        for mode in MODES:
            b = side[mode]
            host, device = [], []
            for r in range(args.repeats):
                row, col = (0, 0) if b == n else (int(rng.integers(0, n - b + 1)), int(rng.integers(0, n - b + 1)))
                block = np.ascontiguousarray(dem[row:row + b, col:col + b] + np.float32(0.5 * (r + 1)))
                h, d, _ = timed(lambda: s.reterrain(block, at=None if b == n else (row, col)))
                host.append(h), device.append(d)
            out[mode] = {"host_ms": stats(host), "device_ms": stats(device), "upload_bytes": int(b * b * 4)}
        s.enqueue_frames(0, 1)  # (the session still renders)
        torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
