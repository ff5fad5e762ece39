"""What horizon rasters on a live session cost (f3d_session_horizon): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM).  Device times are events on the session's stream around the
call, the device warm (two untimed calls first), medians of --repeats.  Everything is in the device form into tensors that
exist, NO_WAIT:
  horizon          --azimuths (default 16) compass azimuths, the K planes written;
  sky_view         the same azimuths, sky_view only (no plane is written);
  visibility x12   what a caller had before: --azimuths x --levels (default 12) launches of f3d_session_raster along
                   (dx_k, s, dz_k), one direction a launch, flat, terrain only, masks out.  A raster's direction is shared by
                   all samples, so this is a LADDER of --levels slopes between the extremes of the horizon planes, not a
                   per-sample bisection: it brackets every sample's horizon to one rung (range / levels), where the planes
                   are exact.  The host decisions between the launches are not timed.
`--block` runs the horizon kernel with a wave owning an 8 x 8 block of samples instead of 64 consecutive ones (the A/B
switch F3D_HORIZON_BLOCK, read when the library first launches a horizon raster: one form per process).

    python tools/horizon_time.py [--dem 2048] [--azimuths 16] [--levels 12] [--repeats 7] [--block]
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
    ap.add_argument("--azimuths", type=int, default=16)
    ap.add_argument("--levels", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--block", action="store_true")
    args = ap.parse_args()
    if args.block:
        os.environ["F3D_HORIZON_BLOCK"] = "1"
    else:
        os.environ.pop("F3D_HORIZON_BLOCK", None)

    import torch

    from forge3d_amd import _native, datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, variance_threshold=1e30, max_frames=4, min_frames=4)
    rows, cols = dem.shape
    n, words, k = rows * cols, (rows * cols + 63) // 64, args.azimuths

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
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    out = {"config": f"rainier proxy {rows}x{cols}, {n} samples, {k} azimuths, {args.levels} levels, medians of {args.repeats}, warm, device events",
           "wave_footprint": "8x8 block" if args.block else "64 consecutive samples"}
    bias = float(np.float32(TerrainSession.SURFACE_BIAS))
    with TerrainSession(dem, args.width, args.height, cam, **kw) as s:
        az = torch.from_numpy(TerrainSession.horizon_directions(k)).cuda()
        planes = torch.zeros((k, n), dtype=torch.float32, device="cuda")
        sky = torch.zeros(n, dtype=torch.float32, device="cuda")

        def horizon(h, v):
            q = _native.HorizonDesc()
            q.struct_size = C.sizeof(_native.HorizonDesc)
            q.flags = _native.HORIZON_DEVICE_POINTERS | _native.HORIZON_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, bias
            q.azimuth_count, q.azimuths = k, az.data_ptr()
            q.horizon, q.sky_view = (h.data_ptr() if h is not None else None), (v.data_ptr() if v is not None else None)
            s._check(s._lib.f3d_session_horizon(s._handle, C.byref(q), s._err, len(s._err)))

        out["horizon_device_ms"] = device_ms(lambda: horizon(planes, None))
        out["sky_view_device_ms"] = device_ms(lambda: horizon(None, sky))
        horizon(planes, sky)
        torch.cuda.synchronize()
        finite = planes[torch.isfinite(planes)]
        out["nan"] = int(torch.isnan(planes).sum())
        out["horizon_min_max"] = [float(finite.min()), float(finite.max())]
        out["sky_view_mean"] = float(sky.mean())

        # the ladder: --levels slopes between the extremes, one direction a launch
        lo, hi = out["horizon_min_max"]
        slopes = np.linspace(lo, hi, args.levels + 2)[1:-1]
        host_az = az.cpu().numpy()
        targets = [[torch.from_numpy(np.array([[host_az[a, 0], sl, host_az[a, 1], 0.0]], np.float32)).cuda() for sl in slopes] for a in range(k)]
        masks = torch.zeros((1, words), dtype=torch.int64, device="cuda")

        def raster(target):
            q = _native.RasterDesc()
            q.struct_size = C.sizeof(_native.RasterDesc)
            q.mode = _native.RASTER_ALONG_DIRECTION
            q.flags = _native.RASTER_TERRAIN_ONLY | _native.RASTER_DEVICE_POINTERS | _native.RASTER_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, bias
            q.target_count, q.targets, q.masks = 1, target.data_ptr(), masks.data_ptr()
            s._check(s._lib.f3d_session_raster(s._handle, C.byref(q), s._err, len(s._err)))

        def ladder():
            for per_azimuth in targets:
                for target in per_azimuth:
                    raster(target)

        out["visibility_ladder_device_ms"] = device_ms(ladder)
        out["visibility_launches"] = k * args.levels
        out["ladder_over_horizon"] = out["visibility_ladder_device_ms"]["median"] / out["horizon_device_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
