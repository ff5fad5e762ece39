"""What shadow-depth rasters on a live session cost (f3d_session_umbra): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM).  Device times are events on the session's stream around the
call, the device warm (two untimed calls first), medians of --repeats; the rows are alternated --rounds times in one process
and each row reports the median of its medians and their range.  Everything is in the device form into tensors that exist,
NO_WAIT, curved (the sun rays' policy):
  umbra x1         one direction, the sun at azimuth 315 and --elevation (default 10) degrees, the plane written;
  umbra x16        a 16-position track from azimuth 100 to 260, its elevation rising from 5 to 45 degrees and back, the 16
                   planes written;
  deepest x16      the same track, `deepest` only (no plane is written);
  shadow mask      the one-direction f3d_session_raster along the first direction, lift = the surface bias, terrain only;
  ladder x12       what a caller had before: --levels (default 12) such launches at lifts between 0 and the largest depth,
                   which bracket every sample's depth to one rung where the plane is exact.  The host decisions between the
                   launches are not timed.
`--rows` runs the umbra kernel with a wave owning 64 consecutive samples instead of an 8 x 8 block (the A/B switch
F3D_UMBRA_BLOCK=0, read when the library first launches an umbra raster: one form per process).

    python tools/umbra_time.py [--dem 2048] [--elevation 10] [--levels 12] [--repeats 7] [--rounds 3] [--rows]
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


def sun(azimuth_deg, elevation_deg):
    az, el = np.radians(azimuth_deg), np.radians(elevation_deg)
    return [np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el), 0.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--elevation", type=float, default=10.0)
    ap.add_argument("--levels", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", action="store_true")
    args = ap.parse_args()
    if args.rows:
        os.environ["F3D_UMBRA_BLOCK"] = "0"
    else:
        os.environ.pop("F3D_UMBRA_BLOCK", None)

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

    out = {"config": f"rainier proxy {rows}x{cols}, {n} samples, sun 315 / {args.elevation:g}, {args.levels} levels, medians of {args.repeats}, "
                     f"{args.rounds} alternated rounds, warm, device events, curved",
           "wave_footprint": "64 consecutive samples" if args.rows else "8x8 block"}
    bias = float(np.float32(TerrainSession.SURFACE_BIAS))
    with TerrainSession(dem, args.width, args.height, cam, **kw) as s:
        track = [sun(100.0 + 160.0 * (i + 0.5) / 16.0, 5.0 + 40.0 * np.sin(np.pi * (i + 0.5) / 16.0)) for i in range(16)]
        one = torch.from_numpy(np.array([sun(315.0, args.elevation)], np.float32)).cuda()
        sixteen = torch.from_numpy(np.array(track, np.float32)).cuda()
        plane = torch.zeros(n, dtype=torch.float32, device="cuda")
        planes = torch.zeros((16, n), dtype=torch.float32, device="cuda")
        deepest = torch.zeros(n, dtype=torch.float32, device="cuda")
        masks = torch.zeros((1, words), dtype=torch.int64, device="cuda")

        def umbra(directions, depth, deep):
            q = _native.UmbraDesc()
            q.struct_size = C.sizeof(_native.UmbraDesc)
            q.flags = _native.UMBRA_CURVED | _native.UMBRA_DEVICE_POINTERS | _native.UMBRA_NO_WAIT
            q.row0, q.col0, q.rows, q.cols = 0, 0, rows, cols
            q.direction_count, q.directions = int(directions.shape[0]), directions.data_ptr()
            q.depth, q.deepest = (depth.data_ptr() if depth is not None else None), (deep.data_ptr() if deep is not None else None)
            s._check(s._lib.f3d_session_umbra(s._handle, C.byref(q), s._err, len(s._err)))

        def raster(lift):
            q = _native.RasterDesc()
            q.struct_size = C.sizeof(_native.RasterDesc)
            q.mode = _native.RASTER_ALONG_DIRECTION
            q.flags = _native.RASTER_TERRAIN_ONLY | _native.RASTER_CURVED | _native.RASTER_DEVICE_POINTERS | _native.RASTER_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, float(lift)
            q.target_count, q.targets, q.masks = 1, one.data_ptr(), masks.data_ptr()
            s._check(s._lib.f3d_session_raster(s._handle, C.byref(q), s._err, len(s._err)))

        umbra(one, plane, None)
        umbra(sixteen, planes, deepest)
        raster(bias)
        torch.cuda.synchronize()
        out["nan"] = int(torch.isnan(plane).sum() + torch.isnan(planes).sum() + torch.isnan(deepest).sum())
        out["umbra_1_max_mean_zero_share"] = [float(plane.max()), float(plane.mean()), float((plane == 0).float().mean())]
        out["deepest_16_max_mean_zero_share"] = [float(deepest.max()), float(deepest.mean()), float((deepest == 0).float().mean())]
        out["deepest_equals_the_maximum_of_the_planes"] = bool(torch.equal(deepest, planes.max(0).values))
        bit = torch.arange(64, dtype=torch.int64, device="cuda")
        lit = (((masks.unsqueeze(-1) >> bit) & 1) != 0).reshape(-1)[:n]
        out["shadow_mask_lit_share"] = float(lit.float().mean())
        h = torch.from_numpy(dem.astype(np.float32)).cuda().reshape(-1) * float(np.float32(kw["exaggeration"]))
        band = 2e-3 * (1.0 + plane + h.abs() + float(h.max() - h.min()))
        decided = (plane - bias).abs() > band
        out["shadow_mask_disagreements_outside_the_band"] = int(((lit != (plane < bias)) & decided).sum())
        out["shadow_mask_share_in_the_band"] = float((~decided).float().mean())
        lifts = np.linspace(0.0, float(plane.max()), args.levels + 2)[1:-1]

        def ladder():
            for lift in lifts:
                raster(lift)

        rows_of = {"umbra_1_device_ms": lambda: umbra(one, plane, None), "umbra_16_planes_device_ms": lambda: umbra(sixteen, planes, None),
                   "umbra_16_deepest_device_ms": lambda: umbra(sixteen, None, deepest), "shadow_mask_device_ms": lambda: raster(bias),
                   "shadow_mask_ladder_device_ms": ladder}
        medians = {name: [] for name in rows_of}
        for _ in range(args.rounds):
            for name, call in rows_of.items():
                medians[name].append(device_ms(call))
        for name, values in medians.items():
            out[name] = {"median": statistics.median(values), "min": min(values), "max": max(values)}
        out["ladder_launches"] = args.levels
        out["umbra_over_shadow_mask"] = out["umbra_1_device_ms"]["median"] / out["shadow_mask_device_ms"]["median"]
        out["ladder_over_umbra"] = out["shadow_mask_ladder_device_ms"]["median"] / out["umbra_1_device_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
