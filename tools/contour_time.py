"""What contour lines cost on a live session (f3d_session_contours, f3d_session_paint_contours), against the route a caller had
before them: one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2) under a --canvas^2 drape (default 4096^2), per interval (--intervals, default 100 and
10, in the unit of the session's heights), warmed (two untimed rounds), the routes ALTERNATING inside every round, medians of
--repeats.  Every figure is host wall time between two device-wide waits around calls that end in a wait themselves:
  contours_ms        contours(): the count call, then the fill call, the segments and level indices in host memory
  count_ms           the count call alone (null outputs: levels up, count pass, scan, the total down), with the band cull: the
                     mean over a window of --count-calls (100) back-to-back calls, each ending in its own wait
  count_nocull_ms    ... and without it (F3D_CONTOUR_CULL=0: every block bisects nothing and every lane walks from all levels)
  paint_contours_ms  paint_contours(): count, emit into the paint buffer, the paint's count / bin / paint, the re-aim pass
  host_route_ms      contours() to the host, then paint(segments): what a caller without paint_contours() pays, given contours()
  paint_ms           the paint's own three device steps inside paint_contours (TerrainSession.paint_stats), summed
The canvas is draped again (untimed) before every painted round, so every round paints the same canvas.  The two painted
routes leave the same bits (checked once per interval).

    python tools/contour_time.py [--dem 2048] [--canvas 4096] [--intervals 100 10] [--repeats 5] [--count-calls 100] [--budget-gib 8]
"""
from __future__ import annotations

import argparse
import json
import os
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
    ap.add_argument("--intervals", type=float, nargs="+", default=[100.0, 10.0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--count-calls", type=int, default=100, help="count calls in one timed window (each ends in a wait for the total)")
    ap.add_argument("--budget-gib", type=int, default=8, help="the session's memory budget: millions of segments need keys beyond the default 512 MiB")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))

    import torch

    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=1, variance_threshold=1e30, max_frames=4, min_frames=4)
    spacing = kw.get("spacing", (1.0, 1.0))
    texel = (dem.shape[1] - 1) * float(spacing[0]) / args.canvas
    image = np.random.default_rng(3).uniform(0.1, 0.9, (args.canvas, args.canvas, 3)).astype(np.float32)
    style = dict(rgba=(0.0, 0.0, 0.0, 0.8), width=1.5 * texel)
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

        def count_only(levels, cull):
            os.environ["F3D_CONTOUR_CULL"] = "1" if cull else "0"
            try:
                return _count(s, levels)
            finally:
                os.environ.pop("F3D_CONTOUR_CULL", None)

        for interval in args.intervals:
            levels = s.contour_levels(interval)
            keys = ("contours_ms", "count_ms", "count_nocull_ms", "paint_contours_ms", "host_route_ms", "paint_ms")
            t = {k: [] for k in keys}
            segments = None
            for r in range(args.repeats + 2):
                ms = {}
                ms["contours_ms"], got = timed(lambda: s.contours(levels))
                # (a count call is a tenth of a millisecond: --count-calls of them in a window, the window's time divided by them)
                ms["count_ms"], total = timed(lambda: [count_only(levels, True) for _ in range(args.count_calls)][-1])
                ms["count_nocull_ms"], total_nocull = timed(lambda: [count_only(levels, False) for _ in range(args.count_calls)][-1])
                ms["count_ms"], ms["count_nocull_ms"] = ms["count_ms"] / args.count_calls, ms["count_nocull_ms"] / args.count_calls
                assert total == total_nocull == got["total"]
                s.drape(image)
                ms["paint_contours_ms"], painted = timed(lambda: s.paint_contours(levels, **style))
                ms["paint_ms"] = sum((s.paint_stats() or {}).get(k, 0.0) for k in ("count_ms", "bin_ms", "paint_ms"))
                if r == 0:
                    direct = s.drape_image().tobytes()
                s.drape(image)

                def host_route():
                    g = s.contours(levels)
                    s.paint(g["segments"].reshape(-1, 2), style["rgba"], np.arange(2 * g["total"], dtype=np.uint32), primitive="lines", width=style["width"])

                ms["host_route_ms"], _ = timed(host_route)
                if r == 0:
                    assert s.drape_image().tobytes() == direct, "the two painted routes leave the same bits"
                segments = painted
                if r >= 2:
                    for k in keys:
                        t[k].append(ms[k])
            out[f"interval_{interval:g}"] = dict(levels=int(levels.size), segments=int(segments), **{k: summary(v) for k, v in t.items()})
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
    print(json.dumps(out))


def _count(s, levels):
    """The count call of contours() alone: f3d_session_contours with null outputs."""
    import ctypes as C

    from forge3d_amd import _native

    total = C.c_uint64(0)
    q = _native.ContoursDesc()
    q.struct_size = C.sizeof(q)
    q.row0, q.col0, q.rows, q.cols = 0, 0, s.dem_shape[0] - 1, s.dem_shape[1] - 1
    q.levels, q.level_count, q.total = levels.ctypes.data, levels.size, C.addressof(total)
    s._check(s._lib.f3d_session_contours(s._handle, C.byref(q), s._err, len(s._err)))
    return int(total.value)


if __name__ == "__main__":
    main()
