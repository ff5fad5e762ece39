"""What painting vector features into the drape costs (f3d_session_paint), against uploading a rasterised image: one GPU, one
job, one JSON line.

The rainier proxy (--dem, default 2048^2) under a --canvas^2 drape (default 4096^2), three workloads:
  segments   --segments (200 000) short segments: seeded random walks of 100 steps, strokes two texels wide, a feature per walk
  triangles  --triangles (100 000) small triangles, a feature each
  polygons   100 wide polygons (fans of 16 triangles, a sixth of the canvas across, opacity 0.5) plus, in a second call, one
             polyline along the full diagonal
Per workload, warmed (two untimed rounds) and ALTERNATING with the comparison, medians of --repeats:
  paint_wall_ms    paint() to the device's end, host wall time: the host scan, the records' upload, binning, the paint kernel
                   and the re-aim pass every update ends with
  count / bin / paint_ms   device events around the three device steps (TerrainSession.paint_stats)
  paint_gb_s       the paint kernel's canvas traffic -- 16 bytes (read + write) per texel of every tile painted -- over paint_ms
  drape_wall_ms    drape() of a --canvas^2 f32 RGB host image, to the device's end: what a caller without paint() pays per change
                   AFTER rasterising on the CPU (the old path without its rasterisation)
A paint call holds host work and two waits for a counter between its device steps, so the whole call is timed as the caller sees
it, by the host's clock between two device-wide waits; the three device steps inside it are events.
--drape-only times drape() alone and --tree DIR imports the package from another checkout: together they time the comparison AT
the parent commit, whose tree has no paint() (run in a process of its own, alternating with this tool by the caller).

    python tools/paint_time.py [--dem 2048] [--canvas 4096] [--repeats 5] [--drape-only] [--tree DIR]
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


def workloads(extent: float, texel: float, segments: int, triangles: int):
    """{name: [paint() keyword sets]} over a square of +-extent metres."""
    rng = np.random.default_rng(17)
    walks = max(segments // 100, 1)
    start = rng.uniform(-0.9 * extent, 0.9 * extent, (walks, 1, 2))
    steps = rng.normal(0.0, 3.0 * texel, (walks, 100, 2))
    path = np.concatenate([start, start + np.cumsum(steps, 1)], 1).astype(np.float32)  # (walks, 101, 2)
    first = (np.arange(walks)[:, None] * 101 + np.arange(100)[None, :]).ravel()
    seg = dict(xz=path.reshape(-1, 2), rgba=rng.uniform(0, 1, (walks * 101, 4)).astype(np.float32),
               indices=np.stack([first, first + 1], 1).astype(np.uint32), primitive="lines", width=2.0 * texel,
               features=np.repeat(np.arange(walks), 101))
    centre = rng.uniform(-0.95 * extent, 0.95 * extent, (triangles, 1, 2))
    tri = dict(xz=(centre + rng.normal(0.0, 4.0 * texel, (triangles, 3, 2))).reshape(-1, 2).astype(np.float32),
               rgba=rng.uniform(0, 1, (triangles * 3, 4)).astype(np.float32), primitive="triangles", features=np.repeat(np.arange(triangles), 3))
    angle = np.linspace(0.0, 2.0 * np.pi, 17)[:-1]
    ring = np.stack([np.cos(angle), np.sin(angle)], 1) * (extent / 6.0)
    centres = rng.uniform(-0.8 * extent, 0.8 * extent, (100, 1, 2))
    verts = np.concatenate([centres, centres + ring[None]], 1).astype(np.float32)  # (100, 17, 2): hub + rim
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 16] for k in range(16)])
    poly = dict(xz=verts.reshape(-1, 2), rgba=np.repeat(rng.uniform(0, 1, (100, 4)), 17, 0).astype(np.float32),
                indices=(np.arange(100)[:, None, None] * 17 + fan[None]).astype(np.uint32), primitive="triangles", opacity=0.5,
                features=np.repeat(np.arange(100), 17))
    line = dict(xz=np.array([[-extent, -extent], [0.1 * extent, -0.1 * extent], [extent, extent]], np.float32), rgba=(0.9, 0.1, 0.1, 1.0),
                primitive="lines", width=3.0 * texel)
    return {"segments": [seg], "triangles": [tri], "polygons": [poly, line]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--canvas", type=int, default=4096)
    ap.add_argument("--segments", type=int, default=200_000)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--drape-only", action="store_true", help="time drape() of the canvas-sized host image alone")
    ap.add_argument("--tree", default=str(ROOT), help="the checkout whose forge3d_amd is imported (default: this one)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.tree).resolve()))

    import torch

    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=1, variance_threshold=1e30, max_frames=4, min_frames=4)
    spacing = kw.get("spacing", (1.0, 1.0))
    extent = 0.5 * (dem.shape[1] - 1) * float(spacing[0])
    texel = (dem.shape[1] - 1) * float(spacing[0]) / args.canvas
    image = np.random.default_rng(3).uniform(0.1, 0.9, (args.canvas, args.canvas, 3)).astype(np.float32)
    out = {"config": f"rainier proxy {dem.shape[0]}x{dem.shape[1]}, canvas {args.canvas}^2 ({image.nbytes >> 20} MiB as f32 RGB), medians of "
                     f"{args.repeats}, warm, alternating"}
    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    with TerrainSession(dem, 256, 144, cam, **kw) as s:
        s.drape(image)
        if args.drape_only:
            times = []
            for r in range(3 * args.repeats + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.drape(image)
                torch.cuda.synchronize()
                if r >= 2:
                    times.append((time.perf_counter() - t0) * 1e3)
            import forge3d_amd

            out.update(tree=str(Path(forge3d_amd.__file__).resolve().parent.parent), has_paint=hasattr(s, "paint"), drape_wall_ms=summary(times))
            print(json.dumps(out))
            return
        for name, calls in workloads(extent, texel, args.segments, args.triangles).items():
            wall, drape, steps = [], [], {"count_ms": [], "bin_ms": [], "paint_ms": []}
            counted = None
            for r in range(args.repeats + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stats = []
                for call in calls:
                    s.paint(**call)
                    stats.append(s.paint_stats())
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                s.drape(image)  # the comparison, alternating: the whole canvas goes up again
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r >= 2:
                    wall.append((t1 - t0) * 1e3)
                    drape.append((t2 - t1) * 1e3)
                    for key in steps:
                        steps[key].append(sum(st[key] for st in stats))
                    counted = {key: sum(st[key] for st in stats) for key in ("primitives", "keys", "tiles")}
            paint_ms = statistics.median(steps["paint_ms"])
            out[name] = dict(counted, paint_wall_ms=summary(wall), drape_wall_ms=summary(drape), **{k: summary(v) for k, v in steps.items()},
                             paint_gb_s=counted["tiles"] * 256 * 16 / (paint_ms * 1e-3) / 1e9)
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
