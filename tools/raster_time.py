"""What DEM visibility rasters on a live session cost (f3d_session_raster): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM).  Device times are events on the session's stream around the
call, the device warm (two untimed calls first), medians of --repeats.  Three rows, each in two forms:
  raster      f3d_session_raster in its device form into tensors that exist (targets up front, masks or count out): the
              kernel builds the rays from the terrain the session holds;
  ray list    the same rays built with torch on the device (the DEM as a tensor, the lattice in f64 and rounded once, the
              contract's arithmetic) and pushed through TerrainSession.occluded() in its device-tensor form -- what a caller
              can do without the raster entry.  `occluded` is the query alone over rays that exist, `build + occluded`
              includes the torch kernels that write them (32 bytes a ray).  The sun-hours row reuses one ray buffer and
              rewrites the direction per direction: 96 x N rays do not fit at once.
  viewshed    one observer --observer-height above the ground at (0.2, 0.1) of the half extent, target height 0, flat;
  sun mask    the session's sun (SESSION_SUN; the ray list takes the same direction), curved;
  sun hours   --directions (default 96) sun directions of a day's arc, curved, count only.
Both forms' answers are compared; `mismatches` must be 0.

    python tools/raster_time.py [--dem 2048] [--directions 96] [--repeats 7]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
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
    ap.add_argument("--directions", type=int, default=96)
    ap.add_argument("--observer-height", type=float, default=50.0)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

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
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    out = {"config": f"rainier proxy {rows}x{cols}, {n} samples, {args.directions} directions, medians of {args.repeats}, warm, device events"}
    with TerrainSession(dem, args.width, args.height, cam, **kw) as s:
        sx, sz = np.float32(kw["spacing"][0]), np.float32(kw["spacing"][1])
        ox, oz = np.float32(-0.5 * (cols - 1.0) * float(sx)), np.float32(-0.5 * (rows - 1.0) * float(sz))
        bias = np.float32(1e-3)

        def raster(mode, flags, lift, targets, masks, count):
            """f3d_session_raster, device form, NO_WAIT, into tensors that exist."""
            q = _native.RasterDesc()
            q.struct_size = C.sizeof(_native.RasterDesc)
            q.mode, q.flags = mode, flags | _native.RASTER_DEVICE_POINTERS | _native.RASTER_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, float(lift)
            if targets is not None:
                q.target_count, q.targets = int(targets.shape[0]), targets.data_ptr()
            q.masks = masks.data_ptr() if masks is not None else None
            q.count = count.data_ptr() if count is not None else None
            s._check(s._lib.f3d_session_raster(s._handle, C.byref(q), s._err, len(s._err)))

        def bits_of(masks):
            bit = torch.arange(64, dtype=torch.int64, device=masks.device)
            return (((masks.unsqueeze(-1) >> bit) & 1) != 0).reshape(masks.shape[0], -1)[:, :n]

        # the ray list a caller builds: the DEM as the session holds it, the lattice rounded once
        heights = torch.from_numpy(dem.astype(np.float32)).cuda() * float(np.float32(kw["exaggeration"]))
        px = (torch.arange(cols, dtype=torch.float64, device="cuda") * float(sx) + float(ox)).float()
        pz = (torch.arange(rows, dtype=torch.float64, device="cuda") * float(sz) + float(oz)).float()
        rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")

        def build_origins(lift):
            rays[:, 0] = px.repeat(rows)
            rays[:, 1] = (heights + float(lift)).reshape(-1)
            rays[:, 2] = pz.repeat_interleave(cols)
            rays[:, 3] = 0.0

        def build_toward(observer):
            build_origins(bias)
            rays[:, 4] = observer[0] - rays[:, 0]
            rays[:, 5] = observer[1] - rays[:, 1]
            rays[:, 6] = observer[2] - rays[:, 2]
            rays[:, 7] = 1.0

        def build_along(direction):
            rays[:, 4], rays[:, 5], rays[:, 6] = float(direction[0]), float(direction[1]), float(direction[2])
            rays[:, 7] = 1e30

        # ---- viewshed: one observer, flat -------------------------------------------------------------------------------------
        xz = np.array([[0.2 * float(-ox), 0.1 * float(-oz)]], np.float32)
        observer = np.array([xz[0, 0], s.ground(xz)[0] + np.float32(args.observer_height), xz[0, 1]], np.float32)
        target = torch.from_numpy(np.array([[*observer, 0.0]], np.float32)).cuda()
        masks = torch.zeros((1, words), dtype=torch.int64, device="cuda")
        out["viewshed_raster_device_ms"] = device_ms(lambda: raster(_native.RASTER_TOWARD_POINT, 0, bias, target, masks, None))
        build_toward(observer)
        out["viewshed_occluded_device_ms"] = device_ms(lambda: s.occluded(rays, wait=False))
        out["viewshed_build_and_occluded_device_ms"] = device_ms(lambda: (build_toward(observer), s.occluded(rays, wait=False)))
        seen = bits_of(masks)[0]
        blocked = s.occluded(rays)
        out["viewshed_visible_fraction"] = float(seen.float().mean())
        out["viewshed_mismatches"] = int((seen == blocked).sum())

        # ---- sun mask: the session's sun, curved -----------------------------------------------------------------------------
        out["sun_mask_raster_device_ms"] = device_ms(
            lambda: raster(_native.RASTER_ALONG_DIRECTION, _native.RASTER_CURVED | _native.RASTER_SESSION_SUN, bias, None, masks, None))
        lit = bits_of(masks)[0].clone()
        az, el = np.radians(kw["sun_azimuth_deg"]), np.radians(kw["sun_elevation_deg"])
        sun = np.array([np.cos(az) * np.cos(el), np.sin(el), np.sin(az) * np.cos(el)], np.float32)  # (to within the last bit of light.wi)
        build_origins(bias)
        build_along(sun)
        out["sun_mask_occluded_device_ms"] = device_ms(lambda: s.occluded(rays, curved=True, wait=False))
        out["sun_mask_build_and_occluded_device_ms"] = device_ms(lambda: (build_origins(bias), build_along(sun), s.occluded(rays, curved=True, wait=False)))
        blocked = s.occluded(rays, curved=True)
        out["sun_mask_lit_fraction"] = float(lit.float().mean())
        out["sun_mask_mismatches_up_to_the_suns_last_bit"] = int((lit == blocked).sum())

        # ---- sun hours: a day's arc, curved, count only ---------------------------------------------------------------------------
        t = np.linspace(0.02, 0.98, args.directions)
        az, el = np.radians(90.0 + 180.0 * t), np.radians(2.0 + 48.0 * np.sin(np.pi * t))
        day = np.stack([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el), np.zeros_like(t)], 1).astype(np.float32)
        d_day = torch.from_numpy(day).cuda()
        count = torch.zeros(n, dtype=torch.int32, device="cuda")
        out["sun_hours_raster_device_ms"] = device_ms(lambda: raster(_native.RASTER_ALONG_DIRECTION, _native.RASTER_CURVED, bias, d_day, None, count))
        hours = torch.zeros(n, dtype=torch.int32, device="cuda")

        def by_ray_list(build):
            hours.zero_()
            if build:
                build_origins(bias)
            for direction in day:
                build_along(direction)
                hours.add_((~s.occluded(rays, curved=True, wait=False)).int())

        build_origins(bias)
        out["sun_hours_build_and_occluded_device_ms"] = device_ms(lambda: by_ray_list(True))
        by_ray_list(False)
        torch.cuda.synchronize()
        out["sun_hours_mean"] = float(count.float().mean())
        out["sun_hours_mismatches"] = int((count != hours).sum())
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
