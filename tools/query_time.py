"""What ray queries on a live session cost (f3d_session_query): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM) at --width x --height (default 1920x1080).  Device times are
events on the session's stream around the call, the device warm (two untimed calls first), medians of --repeats:
  pixels      mode 2 over every pixel of the image, device tensors -- next to a re-aim to the same camera in the same job
              (k_reaim: the same centre rays plus both certificate sets and the clears) and a session create's G-buffer pass;
  ground      --rays (default 1 M) vertical rays in row order, terrain only, device tensors;
  random      --rays rays with random origins above the footprint and random downward directions, device tensors: the
              incoherent case -- the lanes of a wave walk unrelated marches (sorting a batch is not part of the library);
  occluded    the same random rays through the any-hit march;
  host form   wall time of TerrainSession.trace for 1, 1 000 and --rays NumPy rays (staged copies and the blocking wait
              included; the scratch exists after the first call of a size).

    python tools/query_time.py [--dem 2048] [--width 1920] [--height 1080] [--rays 1000000] [--repeats 7]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import torch

    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, variance_threshold=1e30, max_frames=4, min_frames=4)
    W, H, n = args.width, args.height, args.rays
    rng = np.random.default_rng(17)

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

    def wall_ms(call):
        values = []
        for r in range(args.repeats + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if r >= 2:
                values.append((time.perf_counter() - t0) * 1e3)
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    out = {"config": f"rainier proxy {dem.shape[0]}^2, {W}x{H}, {n} rays, medians of {args.repeats}, warm, device events"}
    with TerrainSession(dem, W, H, cam, **kw) as s:
        sx, sz = kw["spacing"]
        half_x, half_z = 0.5 * (dem.shape[1] - 1) * sx, 0.5 * (dem.shape[0] - 1) * sz
        top = float(dem.max()) * kw["exaggeration"]
        pixels = torch.stack(torch.meshgrid(torch.arange(W, dtype=torch.int32), torch.arange(H, dtype=torch.int32), indexing="xy"), -1).reshape(-1, 2).cuda()
        out["pixels_device_ms"] = device_ms(lambda: s.pick(pixels, wait=False))
        out["pixels"] = int(pixels.shape[0])
        hit = s.pick(pixels)["kind"]
        out["pixels_hit_fraction"] = float((hit != 0).float().mean())
        out["reaim_device_ms"] = device_ms(lambda: s.reaim(cam))
        side = int(np.sqrt(n))
        gx, gz = np.meshgrid(np.linspace(-0.999 * half_x, 0.999 * half_x, side), np.linspace(-0.999 * half_z, 0.999 * half_z, side))
        xz = torch.from_numpy(np.stack([gx.ravel(), gz.ravel()], 1).astype(np.float32)).cuda()
        out["ground_rays"] = int(xz.shape[0])
        out["ground_device_ms"] = device_ms(lambda: s.ground(xz))
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0] = rng.uniform(-half_x, half_x, n)
        rays[:, 1] = rng.uniform(1.05, 2.0, n) * top
        rays[:, 2] = rng.uniform(-half_z, half_z, n)
        d = rng.normal(size=(n, 3))
        d[:, 1] = -np.abs(d[:, 1]) * 0.3
        rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays[:, 3], rays[:, 7] = 1e-3, 1e30
        d_rays = torch.from_numpy(rays).cuda()
        out["random_device_ms"] = device_ms(lambda: s.trace(d_rays, wait=False))
        out["random_hit_fraction"] = float((s.trace(d_rays)["kind"] != 0).float().mean())
        order = np.lexsort((np.floor((rays[:, 0] + half_x) / (64 * sx)), np.floor((rays[:, 2] + half_z) / (64 * sz))))
        d_sorted = torch.from_numpy(np.ascontiguousarray(rays[order])).cuda()
        out["random_sorted_by_origin_tile_device_ms"] = device_ms(lambda: s.trace(d_sorted, wait=False))
        out["occluded_random_device_ms"] = device_ms(lambda: s.occluded(d_rays, wait=False))
        for count in (1, 1000, n):
            out[f"host_form_wall_ms_{count}"] = wall_ms(lambda: s.trace(rays[:count]))
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
    # a create's G-buffer pass for the same camera: device time of the whole create (uploads and table build included on a
    # cold DEM; here the DEM is cached, so it is the clears and k_gbuffer)
    def create():
        TerrainSession(dem, W, H, cam, **kw).close()

    out["create_cached_dem_device_ms"] = device_ms(create)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
