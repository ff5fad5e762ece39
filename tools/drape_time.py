"""What an image draped over the terrain costs (f3d_session_drape): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM) at --width x --height (1080p), --spp 8.  Device times are events on
the session's stream, the device warm (two untimed rounds first), medians of --repeats:
  frame         one fused frame (head kernel + frame kernel) of a warm render, frames 4.. of it: undraped, then draped with a
                --small^2 and a --large^2 image (2048^2 and 8192^2), each under the nearest and the bilinear filter;
  ratio         draped / undraped of those medians;
  upload+pack   the drape call itself: the host form (scan, staged upload through the slab, k_drape_pack; host wall time up to
                the device's end) and the device form (k_drape_pack alone over a tensor that exists; device events).
The images are smooth noise (a low-resolution random field, bilinearly enlarged, plus per-texel noise): every texel differs from
its neighbours, so the large image cannot be served from a few cache lines.

    python tools/drape_time.py [--dem 2048] [--small 2048] [--large 8192] [--repeats 7]
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


def noise_image(side: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    coarse = rng.uniform(0.1, 0.8, (65, 65, 3)).astype(np.float32)
    t = np.linspace(0.0, 64.0, side, dtype=np.float32)
    i0 = np.minimum(t.astype(np.int32), 63)
    f = (t - i0)[:, None]
    rows = coarse[i0] * (1 - f[:, :, None]) + coarse[i0 + 1] * f[:, :, None]          # (side, 65, 3)
    image = rows[:, i0] * (1 - f[None, :, :]) + rows[:, i0 + 1] * f[None, :, :]       # (side, side, 3)
    image += rng.uniform(-0.05, 0.05, (side, side, 1)).astype(np.float32)
    return np.ascontiguousarray(np.clip(image, 0.0, 1.0), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--small", type=int, default=2048)
    ap.add_argument("--large", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import torch

    from forge3d_amd import datasets
    from forge3d_amd.session import TerrainSession

    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=args.spp, variance_threshold=1e30, max_frames=64, min_frames=64)
    out = {"config": f"rainier proxy {dem.shape[0]}x{dem.shape[1]}, {args.width}x{args.height}, {args.spp} spp, drapes {args.small}^2 and "
                     f"{args.large}^2, medians of {args.repeats}, warm, device events"}

    def frame_ms(s):
        """Median device time of one frame of a warm render (frames 4..): the render restarts at frame 0 first."""
        s.rearm()
        s.enqueue_frames(0, 4)
        values = []
        for r in range(args.repeats + 2):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.enqueue_frames(4 + r, 1)
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                values.append(e0.elapsed_time(e1))
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    with TerrainSession(dem, args.width, args.height, cam, **kw) as s:
        out["sample_lanes"] = s.sample_lanes()
        base = frame_ms(s)
        out["frame_undraped_ms"] = base
        for name, side in (("small", args.small), ("large", args.large)):
            image = noise_image(side, 7 + side)
            host, device = [], []
            for r in range(args.repeats + 2):  # the host form: scan + staged upload + pack, to the device's end
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.drape(image)
                torch.cuda.synchronize()
                if r >= 2:
                    host.append((time.perf_counter() - t0) * 1e3)
            d_image = torch.from_numpy(image).cuda()
            for r in range(args.repeats + 2):  # the device form: the packing kernel (and the re-aim pass every update ends with)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s.drape(d_image, wait=False)
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    device.append(e0.elapsed_time(e1))
            del d_image
            out[f"drape_{name}_side"] = side
            out[f"drape_{name}_bytes"] = s.drape_info()["bytes"]
            out[f"drape_{name}_host_form_wall_ms"] = {"median": statistics.median(host), "min": min(host), "max": max(host)}
            out[f"drape_{name}_device_form_device_ms"] = {"median": statistics.median(device), "min": min(device), "max": max(device)}
            for filt in ("nearest", "bilinear"):
                s.drape(image, filter=filt)
                t = frame_ms(s)
                out[f"frame_{name}_{filt}_ms"] = t
                out[f"ratio_{name}_{filt}"] = t["median"] / base["median"]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.reaim(cam)
        e1.record()
        torch.cuda.synchronize()
        out["reaim_pass_device_ms"] = e0.elapsed_time(e1)  # (what every update ends with: part of the device-form figures)
        s.drape(None)
        out["frame_undraped_again_ms"] = frame_ms(s)
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
