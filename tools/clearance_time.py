"""What clearance rasters on a live session cost (f3d_session_clearance): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM).  Device times are events on the session's stream around the
call, the device warm (two untimed calls first), medians of --repeats; the rows are alternated --rounds times in one process
and each row reports the median of its medians and their range.  Everything is in the device form into tensors that exist,
NO_WAIT, flat:
  clearance x1     one observer --observer-height above the ground at (0.2, 0.1) of the half extent (tools/raster_time.py's
                   viewshed observer), the plane written;
  clearance x16    that observer and 15 more on a 4 x 4 grid over the footprint, `lowest` only (no plane is written);
  viewshed         the one-observer f3d_session_raster toward the same observer, lift = the surface bias, terrain only;
  ladder x12       what a caller had before: --levels (default 12) such launches at lifts between 0 and the largest finite
                   clearance, which bracket every sample's clearance to one rung where the plane is exact.  The host
                   decisions between the launches are not timed.
`--rows` runs the clearance kernel with a wave owning 64 consecutive samples instead of an 8 x 8 block (the A/B switch
F3D_CLEARANCE_BLOCK=0, read when the library first launches a clearance raster: one form per process).

    python tools/clearance_time.py [--dem 2048] [--levels 12] [--repeats 7] [--rounds 3] [--rows]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--observer-height", type=float, default=50.0)
    ap.add_argument("--levels", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", action="store_true")
    args = ap.parse_args()
    if args.rows:
        os.environ["F3D_CLEARANCE_BLOCK"] = "0"
    else:
        os.environ.pop("F3D_CLEARANCE_BLOCK", None)

    import torch

    from forge3d_amd import _native, datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, variance_threshold=1e30, max_frames=4, min_frames=4)
    rows, cols = dem.shape
    n, words = rows * cols, (rows * cols + 63) // 64

    def device_ms(call):
        values = []
        for r in range(args.repeats + 2):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                values.append(e0.elapsed_time(e1))
        return statistics.median(values)

    out = {"config": f"rainier proxy {rows}x{cols}, {n} samples, {args.levels} levels, medians of {args.repeats}, {args.rounds} alternated rounds, warm, device events",
           "wave_footprint": "64 consecutive samples" if args.rows else "8x8 block"}
    bias = float(np.float32(TerrainSession.SURFACE_BIAS))
    with TerrainSession(dem, args.width, args.height, cam, **kw) as s:
        sx, sz = float(np.float32(kw["spacing"][0])), float(np.float32(kw["spacing"][1]))
        hx, hz = 0.5 * (cols - 1.0) * sx, 0.5 * (rows - 1.0) * sz
        grid = [(fx * hx, fz * hz) for fz in (-0.6, -0.2, 0.2, 0.6) for fx in (-0.6, -0.2, 0.2, 0.6)]
        xz = np.array([(0.2 * hx, 0.1 * hz)] + grid[:15], np.float32)
        y = s.ground(xz) + np.float32(args.observer_height)
        host_observers = np.stack([xz[:, 0], y, xz[:, 1], np.zeros(len(xz), np.float32)], 1).astype(np.float32)
        observers = torch.from_numpy(host_observers).cuda()
        plane = torch.zeros(n, dtype=torch.float32, device="cuda")
        lowest = torch.zeros(n, dtype=torch.float32, device="cuda")
        masks = torch.zeros((1, words), dtype=torch.int64, device="cuda")

        def clearance(k, height, low):
            q = _native.ClearanceDesc()
            q.struct_size = C.sizeof(_native.ClearanceDesc)
            q.flags = _native.CLEARANCE_DEVICE_POINTERS | _native.CLEARANCE_NO_WAIT
            q.row0, q.col0, q.rows, q.cols = 0, 0, rows, cols
            q.observer_count, q.observers = k, observers.data_ptr()
            q.height, q.lowest = (height.data_ptr() if height is not None else None), (low.data_ptr() if low is not None else None)
            s._check(s._lib.f3d_session_clearance(s._handle, C.byref(q), s._err, len(s._err)))

        def raster(lift):
            q = _native.RasterDesc()
            q.struct_size = C.sizeof(_native.RasterDesc)
            q.mode = _native.RASTER_TOWARD_POINT
            q.flags = _native.RASTER_TERRAIN_ONLY | _native.RASTER_DEVICE_POINTERS | _native.RASTER_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, float(lift)
            q.target_count, q.targets, q.masks = 1, observers.data_ptr(), masks.data_ptr()
            s._check(s._lib.f3d_session_raster(s._handle, C.byref(q), s._err, len(s._err)))

        clearance(1, plane, None)
        clearance(len(xz), None, lowest)
        raster(bias)
        torch.cuda.synchronize()
        finite = plane[torch.isfinite(plane)]
        out["nan"] = int(torch.isnan(plane).sum() + torch.isnan(lowest).sum())
        out["clearance_1_max_mean_zero_share"] = [float(finite.max()), float(finite.mean()), float((plane == 0).float().mean())]
        out["clearance_16_zero_share"] = float((lowest == 0).float().mean())
        bit = torch.arange(64, dtype=torch.int64, device="cuda")
        seen = (((masks.unsqueeze(-1) >> bit) & 1) != 0).reshape(-1)[:n]
        out["viewshed_visible_share"] = float(seen.float().mean())
        band = 2e-3 * (1.0 + plane.abs() + abs(float(y[0])) + torch.from_numpy(dem.astype(np.float32)).cuda().reshape(-1).abs() * float(np.float32(kw["exaggeration"])))
        decided = torch.isfinite(plane) & ((plane - bias).abs() > band)
        out["viewshed_disagreements_outside_the_band"] = int(((seen != (plane < bias)) & decided).sum())
        lifts = np.linspace(0.0, float(finite.max()), args.levels + 2)[1:-1]

        def ladder():
            for lift in lifts:
                raster(lift)

        rows_of = {"clearance_1_device_ms": lambda: clearance(1, plane, None), "clearance_16_lowest_device_ms": lambda: clearance(len(xz), None, lowest),
                   "viewshed_device_ms": lambda: raster(bias), "viewshed_ladder_device_ms": ladder}
        medians = {name: [] for name in rows_of}
        for _ in range(args.rounds):
            for name, call in rows_of.items():
                medians[name].append(device_ms(call))
        for name, values in medians.items():
            out[name] = {"median": statistics.median(values), "min": min(values), "max": max(values)}
        out["ladder_launches"] = args.levels
        out["clearance_over_viewshed"] = out["clearance_1_device_ms"]["median"] / out["viewshed_device_ms"]["median"]
        out["ladder_over_clearance"] = out["viewshed_ladder_device_ms"]["median"] / out["clearance_1_device_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
