"""Time a camera orbit of the rainier-proxy terrain two ways on one GPU, in one run, and print one JSON line.

A 24-key orbit of the 2048^2 rainier proxy at 1920x1080, 8 accumulation frames of 8 spp a key, through the public wrapper,
after two keys of warm-up each:
  oneshot   hybrid_render_terrain_reference per key (what ViewerHandle.render_animation did per keyframe: validate, hash
            the DEM for the scene cache, allocate and clear the per-pixel state, streams and events, G-buffer pass, render,
            free) -- repeated --repeats times for its spread;
  reaim     render_terrain_camera_sequence: one session, re-aimed per key (f3d_session_reaim).
Wall time per key, readback into numpy included in both.

    python tools/camera_sequence_time.py [--keys 24] [--warmup 2] [--repeats 3] [--dem 2048] [--width 1920 --height 1080]

Device time of the re-aim pass against a create's G-buffer pass and clears: run the tool once under
`rocprofv3 --kernel-trace --stats -d DIR -o cam -- python tools/camera_sequence_time.py --keys 4 --repeats 1`, then
    python tools/camera_sequence_time.py --trace-db DIR
prints the kernels' times from the trace database (one JSON line).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def trace_summary(root: str) -> dict:
    """k_reaim, k_gbuffer, k_rearm and the memset kernels of a rocprofv3 --kernel-trace database under `root`."""
    import sqlite3

    dbs = sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 database under {root}")
    cur = sqlite3.connect(dbs[0]).cursor()
    rows = cur.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    out = {"database": os.path.relpath(dbs[0], root)}

    def pick(label, match):
        hit = [r for r in rows if match(r[0])]
        calls = sum(r[1] for r in hit)
        total = sum(r[2] for r in hit)
        out[label] = {"calls": calls, "total_ms": total / 1e6, "avg_ms": total / 1e6 / calls if calls else None,
                      "min_ms": min(r[4] for r in hit) / 1e6 if hit else None, "max_ms": max(r[5] for r in hit) / 1e6 if hit else None}
        return out[label]

    reaim = pick("k_reaim", lambda n: "k_reaim" in n)
    gbuffer = pick("k_gbuffer", lambda n: "k_gbuffer" in n)
    pick("k_trace_init", lambda n: "k_trace_init" in n)
    fills = pick("memset_kernels", lambda n: "fillBuffer" in n or "memset" in n.lower())
    if gbuffer["calls"]:
        # (every memset kernel of the run over the creates of the run: the frame loop's 8-byte stats clears are in it)
        out["memsets_ms_per_create"] = fills["total_ms"] / gbuffer["calls"]
        out["create_device_ms"] = gbuffer["avg_ms"] + out["memsets_ms_per_create"]
    if reaim["calls"] and gbuffer["calls"]:
        out["reaim_minus_gbuffer_ms"] = reaim["avg_ms"] - gbuffer["avg_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="repeats of the one-shot form (its spread)")
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--accum", type=int, default=8, help="accumulation frames per key")
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--trace-db", default=None, help="summarise a rocprofv3 --kernel-trace database directory instead")
    args = ap.parse_args()
    if args.trace_db:
        print(json.dumps(trace_summary(args.trace_db)))
        return

    from forge3d_amd import datasets
    from forge3d_amd.path_tracing import hybrid_render_terrain_reference, render_terrain_camera_sequence

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=args.spp, variance_threshold=1e30, max_frames=args.accum, min_frames=args.accum)
    W, H = args.width, args.height
    span = (args.dem - 1) * kw["spacing"][0]
    target = tuple(cam["look_at"])
    n = args.warmup + args.keys
    cameras = [datasets.orbit_camera(target, 1.25 * span, 28.0 + 360.0 * i / args.keys, 49.0, 42.0) for i in range(n)]

    def oneshots():
        stamps = [time.perf_counter()]
        for c in cameras:
            hybrid_render_terrain_reference(dem, W, H, c, **kw)
            stamps.append(time.perf_counter())
        return (stamps[-1] - stamps[args.warmup]) * 1e3 / args.keys

    def sequence():
        stamps = [time.perf_counter()]
        for _ in render_terrain_camera_sequence(dem, W, H, frames=[{"camera": c} for c in cameras], **kw):
            stamps.append(time.perf_counter())
        return (stamps[-1] - stamps[args.warmup]) * 1e3 / args.keys

    out = {"config": f"camera orbit: rainier proxy {args.dem}^2, {W}x{H}, {args.accum} frames x {args.spp} spp a key, {args.keys} keys after "
                     f"{args.warmup} of warm-up, through the wrapper, readback included"}
    a = [oneshots() for _ in range(args.repeats)]
    b = sequence()
    out["oneshot_ms_per_key"] = a
    out["oneshot_ms_per_key_median"] = sorted(a)[len(a) // 2]
    out["oneshot_spread_ms"] = max(a) - min(a)
    out["reaim_ms_per_key"] = b
    out["saving_ms_per_key"] = out["oneshot_ms_per_key_median"] - b
    print(json.dumps(out))


if __name__ == "__main__":
    main()
