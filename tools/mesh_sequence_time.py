"""Time an animation of buildings growing on the rainier-proxy terrain two ways on one GPU and print one JSON line.

The 2048^2 rainier proxy with datasets.proxy_buildings (50 000 boxes, 600 000 triangles) at 1920x1080; 24 keys, in each
key a tenth of the boxes rises by a few metres; 8 accumulation frames of 8 spp a key, through the public wrapper, after two
keys of warm-up:
  oneshot   hybrid_render_terrain_reference per key (per key: hash and upload the mesh, the host SAH build, a create with
            its allocations, a destroy) -- this mode uses nothing but the public one-shot call, so it also runs on a
            commit without the re-mesh;
  session   render_terrain_mesh_sequence: one session, re-meshed per key (f3d_session_remesh: vertices uploaded in
            stream order, the BVH refitted on the GPU).
Wall time per key, readback into numpy included in both, --repeats times each.  The session mode also times the frame
kernel (hipEvents around each launch, f3d_session_kernel_timing) on the tree refitted through every key and on the tree
a fresh session builds at the last key's positions: what the kept topology costs.

    python tools/mesh_sequence_time.py [--mode both|oneshot|session] [--keys 24] [--warmup 2] [--repeats 3]

Device time of the refit kernels: run the tool once, with nothing else in the run, under
`rocprofv3 --kernel-trace --stats -d DIR -o mesh -- python tools/mesh_sequence_time.py --mode session --repeats 1`, then
    python tools/mesh_sequence_time.py --trace-db DIR
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

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def trace_summary(root: str) -> dict:
    """The refit kernels, k_reaim and the frame kernels of a rocprofv3 --kernel-trace database under `root`."""
    import sqlite3

    dbs = sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 database under {root}")
    cur = sqlite3.connect(dbs[0]).cursor()
    rows = cur.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name").fetchall()
    out = {"database": os.path.relpath(dbs[0], root)}
    for label in ("k_remesh_gather", "k_remesh_link", "k_remesh_refit_wide", "k_remesh_refit_binary", "k_reaim", "k_gbuffer", "k_frame"):
        hit = [r for r in rows if label in r[0]]
        calls = sum(r[1] for r in hit)
        total = sum(r[2] for r in hit)
        out[label] = {"calls": calls, "total_ms": total / 1e6, "avg_ms": total / 1e6 / calls if calls else None,
                      "min_ms": min(r[4] for r in hit) / 1e6 if hit else None, "max_ms": max(r[5] for r in hit) / 1e6 if hit else None}
    refits = out["k_remesh_gather"]["calls"]
    if refits:
        out["refit_device_ms_per_key"] = sum(out[k]["total_ms"] for k in ("k_remesh_gather", "k_remesh_refit_wide", "k_remesh_refit_binary")) / refits
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("both", "oneshot", "session"), default="both")
    ap.add_argument("--keys", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--accum", type=int, default=8, help="accumulation frames per key")
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--boxes", type=int, default=50_000)
    ap.add_argument("--trace-db", default=None, help="summarise a rocprofv3 --kernel-trace database directory instead")
    args = ap.parse_args()
    if args.trace_db:
        print(json.dumps(trace_summary(args.trace_db)))
        return

    from forge3d_amd import datasets
    from forge3d_amd.path_tracing import hybrid_render_terrain_reference

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=args.spp, variance_threshold=1e30, max_frames=args.accum, min_frames=args.accum)
    W, H = args.width, args.height
    v0, tris = datasets.proxy_buildings(dem, kw["spacing"][0], n_boxes=args.boxes)
    boxes = len(v0) // 8
    n = args.warmup + args.keys
    rng = np.random.default_rng(11)
    lift = rng.uniform(2.0, 4.0, boxes).astype(np.float32)
    positions, v = [], v0.copy()
    for k in range(n):  # key k: every tenth box, starting at k, rises by its 2..4 m (the top four of a box's eight vertices)
        if k:
            v = v.copy()
            rising = np.arange(k % 10, boxes, 10)
            v.reshape(boxes, 8, 3)[rising, 4:, 1] += lift[rising, None]
        positions.append(v)

    def per_key(stamps):
        return (stamps[-1] - stamps[args.warmup]) * 1e3 / args.keys

    out = {"config": f"growing buildings: rainier proxy {args.dem}^2, {len(tris)} triangles, {W}x{H}, {args.accum} frames x {args.spp} spp a key, "
                     f"{args.keys} keys after {args.warmup} of warm-up, through the wrapper, readback included"}
    if args.mode in ("both", "oneshot"):
        runs = []
        for _ in range(args.repeats):
            stamps = [time.perf_counter()]
            for p in positions:
                hybrid_render_terrain_reference(dem, W, H, cam, mesh_vertices=p, mesh_indices=tris, **kw)
                stamps.append(time.perf_counter())
            runs.append(per_key(stamps))
        out["oneshot_ms_per_key"] = runs
    if args.mode in ("both", "session"):
        from forge3d_amd.path_tracing import render_terrain_mesh_sequence
        from forge3d_amd.session import TerrainSession

        runs = []
        for _ in range(args.repeats):
            stamps = [time.perf_counter()]
            frames = [{}] + [{"mesh_vertices": p} for p in positions[1:]]
            for _ in render_terrain_mesh_sequence(dem, W, H, cam, frames=frames, mesh_vertices=v0, mesh_indices=tris, **kw):
                stamps.append(time.perf_counter())
            runs.append(per_key(stamps))
        out["session_ms_per_key"] = runs
        if "oneshot_ms_per_key" in out:
            out["session_slowest_minus_oneshot_fastest_ms"] = max(runs) - min(out["oneshot_ms_per_key"])

        # the frame kernel on the tree refitted through every key against a fresh tree at the last key's positions
        def frame_ms(session):
            session.enqueue_frames(0, 2)  # (warm-up; also the tile order's first costs)
            session.kernel_timing(True)
            session.enqueue_frames(2, args.accum)
            return session.kernel_timing(False)[0]

        with TerrainSession(dem, W, H, cam, mesh_vertices=v0, mesh_indices=tris, **kw) as s:
            for p in positions[1:]:
                s.remesh(p)
            out["frame_ms_refitted_tree"] = frame_ms(s)
        with TerrainSession(dem, W, H, cam, mesh_vertices=positions[-1], mesh_indices=tris, **kw) as s:
            out["frame_ms_fresh_tree"] = frame_ms(s)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
