"""Time a sun sweep of the configs[4] terrain workload two ways on one GPU, in one run, and print one JSON line.

BASELINE.json configs[4] gives every frame of a 120-frame sequence its own 64-spp terrain render (8 accumulation frames of
8 spp, 1920x1080, rainier proxy), the sun's azimuth advancing 0.25 degrees a frame, each render resolved on the device
into the frame's image.  Here the terrain renders alone (no smoke), after a warm-up:
  fresh   a new TerrainSession per frame, created while the frame before still renders and closed once the next one
          exists (the pipelining of bench.py's C5_with_terrain);
  rearm   one session, re-armed per frame (TerrainSession.rearm: the smoke sequence's terrain_sun_provider).
Also the device time of one re-arm pass and of a create's device work (the clears and the G-buffer pass, the scene cached),
each bracketed by events on an otherwise idle stream.

    python tools/sun_sequence_time.py [--frames 120] [--warmup 8] [--dem 2048] [--width 1920 --height 1080]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--accum", type=int, default=8, help="accumulation frames per render")
    ap.add_argument("--spp", type=int, default=8)
    args = ap.parse_args()

    import torch

    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=args.spp, variance_threshold=1e30, max_frames=args.accum, min_frames=args.accum)
    az0 = float(kw.pop("sun_azimuth_deg"))
    W, H, n = args.width, args.height, args.accum
    stream = torch.cuda.Stream()
    base = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    opts = dict(stream=stream.cuda_stream, memory_budget_bytes=8 << 30)

    def fresh_frames(first, count):
        held = None
        for i in range(first, first + count):
            s = TerrainSession(dem, W, H, cam, sun_azimuth_deg=az0 + 0.25 * (i + 1), **opts, **kw)
            if held is not None:
                held.close()
            s.enqueue_frames(0, n)
            s.resolve_device(n, d_rgba=base.data_ptr())
            held = s
        held.close()

    def rearm_frames(s, first, count):
        for i in range(first, first + count):
            s.rearm(sun_azimuth_deg=az0 + 0.25 * (i + 1))
            s.enqueue_frames(0, n)
            s.resolve_device(n, d_rgba=base.data_ptr())
        stream.synchronize()

    out = {"config": f"configs[4] terrain part: rainier proxy {args.dem}^2, {W}x{H}, {n} frames x {args.spp} spp a render, "
                     f"azimuth +0.25 deg a render, {args.frames} renders after {args.warmup} of warm-up, no smoke"}
    fresh_frames(0, args.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh_frames(args.warmup, args.frames)
    torch.cuda.synchronize()
    out["fresh_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / args.frames

    s = TerrainSession(dem, W, H, cam, sun_azimuth_deg=az0, **opts, **kw)
    rearm_frames(s, 0, args.warmup)
    t0 = time.perf_counter()
    rearm_frames(s, args.warmup, args.frames)
    out["rearm_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / args.frames

    # device time of one re-arm pass, and of a create's device work, each alone on the idle stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = []
    for i in range(10):
        stream.synchronize()
        e0.record(stream)
        s.rearm(sun_azimuth_deg=az0 + 7.0 + i)
        e1.record(stream)
        e1.synchronize()
        samples.append(e0.elapsed_time(e1))
    out["rearm_pass_ms"] = sorted(samples)[len(samples) // 2]
    s.close()
    samples = []
    for i in range(5):
        torch.cuda.synchronize()
        e0.record(stream)
        s2 = TerrainSession(dem, W, H, cam, sun_azimuth_deg=az0 + 3.0 + i, **opts, **kw)
        e1.record(stream)
        e1.synchronize()
        samples.append(e0.elapsed_time(e1))
        s2.close()
    out["create_device_ms"] = sorted(samples)[len(samples) // 2]
    out["create_device_ms_note"] = ("events around a create on its stream, the DEM's tables cached: the clears and the G-buffer "
                                    "pass, plus the host time of the create where the stream waited on it (an upper bound)")
    out["saving_ms_per_frame"] = out["fresh_ms_per_frame"] - out["rearm_ms_per_frame"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
