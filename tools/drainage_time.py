"""What drainage costs on a live session (f3d_session_drainage, f3d_session_streams, f3d_session_paint_streams): one GPU, one job,
one JSON line.

The rainier proxy (--dem, default 2048^2) under a --canvas^2 drape (default 4096^2), warmed (two untimed rounds), the routes
ALTERNATING inside every round, medians of --repeats.  Every figure but the split is host wall time between two device-wide
waits around calls that end in a wait themselves:
  drainage_ms        drainage(out="device"): directions, accumulation and basins of the whole DEM into tensors, to the device's end
  direction_ms       ... of it the direction pass, and
  rounds_ms          ... the doubling rounds (each with its counter read back), as the library's own host clock splits them
  rounds, longest    the rounds that had a live sample, the longest path in steps; sinks
  streams_ms         streams(threshold) to the host, per threshold (--thresholds, default 1000 and 100)
  paint_streams_ms   paint_streams(threshold): route, count, emit into the paint buffer, the paint's count / bin / paint, the re-aim pass
  host_route_ms      streams() to the host, then paint(segments): what a caller without paint_streams() pays
With the fill (f3d_session_fill, F3D_DRAINAGE_FILL), beside those rows:
  fill_ms            fill(out="device"): the filled surface, the lakes' depth and the flat distance of the whole DEM into tensors
  fill_pass_ms       ... of it the fill pass (z, W0, the tiled relaxation of W with a counter read back after every round), and
  flat_pass_ms       ... the flat pass (T0, the relaxation of T), as the library's own host clock splits them
  fill_rounds, flat_rounds, filled_samples, largest_flat_distance
  filled_drainage_ms filled.drainage(out="device"): both passes, the direction pass on the filled surface, the doubling rounds;
                     filled_rounds, filled_longest, filled_sinks
  filled_paint_streams_ms, filled_segments   per threshold: paint_streams(threshold, fill=True)
The canvas is draped again (untimed) before every painted round; the two painted routes leave the same bits (checked once per
threshold).  For orientation only (--cpu 1, the default): cpu_sweep_ms, the host build of the same lane bodies
(tests/drainage_host) routing the same DEM serially on one CPU thread, once, and cpu_fill_ms, the host build of the fill's bodies
(tests/fill_host: both passes, tiles in index order) on one thread, once.

    python tools/drainage_time.py [--dem 2048] [--canvas 4096] [--thresholds 1000 100] [--repeats 5] [--budget-gib 8] [--cpu 1]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--canvas", type=int, default=4096)
    ap.add_argument("--thresholds", type=int, nargs="+", default=[1000, 100])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget-gib", type=int, default=8, help="the session's memory budget: the routing's planes are 21 bytes a DEM sample, 33 with the fill")
    ap.add_argument("--cpu", type=int, default=1, help="1: also route the DEM once through the host build of the lane bodies, on one thread")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))

    import torch

    from forge3d_amd import _native, datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=1, variance_threshold=1e30, max_frames=4, min_frames=4)
    spacing = kw.get("spacing", (1.0, 1.0))
    texel = (dem.shape[1] - 1) * float(spacing[0]) / args.canvas
    image = np.random.default_rng(3).uniform(0.1, 0.9, (args.canvas, args.canvas, 3)).astype(np.float32)
    style = dict(rgba=(0.1, 0.3, 0.8, 1.0), width=1.5 * texel)
    out = {"config": f"rainier proxy {dem.shape[0]}x{dem.shape[1]}, canvas {args.canvas}^2, medians of {args.repeats}, warm, alternating"}
    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, got

    with TerrainSession(dem, 256, 144, cam, memory_budget_bytes=args.budget_gib << 30, **kw) as s:
        s.drape(image)
        device = torch.device("cuda", torch.cuda.current_device())
        planes = {"direction": torch.empty(dem.shape, dtype=torch.uint8, device=device), "accumulation": torch.empty(dem.shape, dtype=torch.int32, device=device),
                  "basin": torch.empty(dem.shape, dtype=torch.int32, device=device)}

        def split():
            """One raw call with the library's own clock: (direction pass, rounds) in ms."""
            stats, ms = (C.c_uint32 * 3)(), (C.c_double * 2)()
            q = _native.DrainageDesc()
            q.struct_size = C.sizeof(q)
            q.flags = _native.DRAINAGE_DEVICE_POINTERS
            q.row0, q.col0, q.rows, q.cols = 0, 0, dem.shape[0], dem.shape[1]
            q.accumulation = planes["accumulation"].data_ptr()
            q.stats, q.ms = C.addressof(stats), C.addressof(ms)
            s._check(s._lib.f3d_session_drainage(s._handle, C.byref(q), s._err, len(s._err)))
            return ms[0], ms[1]

        t = {k: [] for k in ("drainage_ms", "direction_ms", "rounds_ms")}
        for r in range(args.repeats + 2):
            whole, got = timed(lambda: s.drainage(basin=True, out=planes))
            torch.cuda.synchronize()
            direction_ms, rounds_ms = split()
            if r >= 2:
                t["drainage_ms"].append(whole), t["direction_ms"].append(direction_ms), t["rounds_ms"].append(rounds_ms)
        out.update({k: summary(v) for k, v in t.items()}, rounds=got["rounds"], longest=got["longest"], sinks=got["sinks"])
        out["accumulation_max"] = int(planes["accumulation"].max().item())

        filled = {"filled": torch.empty(dem.shape, dtype=torch.float32, device=device), "depth": torch.empty(dem.shape, dtype=torch.float32, device=device),
                  "flat_distance": torch.empty(dem.shape, dtype=torch.int32, device=device)}

        def fill_split():
            """One raw call with the library's own clock: (fill pass, flat pass) in ms."""
            ms = (C.c_double * 2)()
            q = _native.FillDesc()
            q.struct_size = C.sizeof(q)
            q.flags = _native.FILL_DEVICE_POINTERS
            q.row0, q.col0, q.rows, q.cols = 0, 0, dem.shape[0], dem.shape[1]
            q.filled = filled["filled"].data_ptr()
            q.ms = C.addressof(ms)
            s._check(s._lib.f3d_session_fill(s._handle, C.byref(q), s._err, len(s._err)))
            return ms[0], ms[1]

        t = {k: [] for k in ("fill_ms", "fill_pass_ms", "flat_pass_ms", "filled_drainage_ms")}
        for r in range(args.repeats + 2):
            whole, got = timed(lambda: s.fill(depth=True, flat_distance=True, out=filled))
            fill_pass_ms, flat_pass_ms = fill_split()
            routed_ms, routed = timed(lambda: s.filled.drainage(basin=True, out=planes))
            if r >= 2:
                t["fill_ms"].append(whole), t["fill_pass_ms"].append(fill_pass_ms), t["flat_pass_ms"].append(flat_pass_ms), t["filled_drainage_ms"].append(routed_ms)
        out.update({k: summary(v) for k, v in t.items()}, fill_rounds=got["fill_rounds"], flat_rounds=got["flat_rounds"], filled_samples=got["filled_samples"],
                   largest_flat_distance=got["largest_flat_distance"], filled_rounds=routed["rounds"], filled_longest=routed["longest"], filled_sinks=routed["sinks"])
        out["filled_accumulation_max"] = int(planes["accumulation"].max().item())

        for threshold in args.thresholds:
            keys = ("streams_ms", "paint_streams_ms", "host_route_ms", "filled_paint_streams_ms")
            t = {k: [] for k in keys}
            for r in range(args.repeats + 2):
                ms = {}
                ms["streams_ms"], got = timed(lambda: s.streams(threshold))
                s.drape(image)
                ms["paint_streams_ms"], painted = timed(lambda: s.paint_streams(threshold, **style))
                if r == 0:
                    direct = s.drape_image().tobytes()
                s.drape(image)

                def host_route():
                    g = s.streams(threshold)
                    if g["total"]:
                        s.paint(g["segments"].reshape(-1, 2), style["rgba"], np.arange(2 * g["total"], dtype=np.uint32), primitive="lines", width=style["width"])

                ms["host_route_ms"], _ = timed(host_route)
                if r == 0:
                    assert s.drape_image().tobytes() == direct, "the two painted routes leave the same bits"
                assert painted == got["total"]
                s.drape(image)
                ms["filled_paint_streams_ms"], filled_segments = timed(lambda: s.paint_streams(threshold, fill=True, **style))
                if r >= 2:
                    for k in keys:
                        t[k].append(ms[k])
            out[f"threshold_{threshold}"] = dict(segments=int(got["total"]), filled_segments=int(filled_segments), **{k: summary(v) for k, v in t.items()})
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
        out["scratch_bytes_per_sample"] = 21
        out["filled_scratch_bytes_per_sample"] = 33

    if args.cpu:
        sys.path.insert(0, str(ROOT / "tests"))
        import drainage_cases as cases

        # (only the terrain matters to the routing: whatever else the emulator's scene wants gets a plain value)
        plain = dict(spacing=(1.0, 1.0), exaggeration=1.0, albedo=(0.6, 0.6, 0.6), sun_azimuth_deg=135.0, sun_elevation_deg=45.0, sun_intensity=1.0,
                     env_intensity=1.0, seed=0, earth_model="flat", refraction_model="none")
        host = cases.HostDrainage(cases.build_harness(), dem, dict(plain, **kw), cam)
        try:
            t0 = time.perf_counter()
            cpu = host.run((0, 0, 1, 1))  # (routes the whole DEM; one sample written back)
            out["cpu_sweep_ms"] = (time.perf_counter() - t0) * 1e3
            assert (cpu["rounds"], cpu["longest"], cpu["sinks"]) == (out["rounds"], out["longest"], out["sinks"])
        finally:
            host.close()
        import fill_cases

        host = fill_cases.HostFill(fill_cases.build_harness(), dem, dict(plain, **kw), cam)
        try:
            t0 = time.perf_counter()
            cpu = host.fill((0, 0, 1, 1))  # (both passes over the whole DEM; one sample written back)
            out["cpu_fill_ms"] = (time.perf_counter() - t0) * 1e3
            out["cpu_fill_rounds"], out["cpu_flat_rounds"] = cpu["fill_rounds"], cpu["flat_rounds"]
            assert (cpu["filled_samples"], cpu["largest_flat_distance"]) == (out["filled_samples"], out["largest_flat_distance"])
        finally:
            host.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
