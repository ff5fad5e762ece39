"""What an irradiation raster on a live session costs (f3d_session_irradiation): one GPU, one job, one JSON line.

The rainier proxy (--dem, default 2048^2: the headline DEM), --directions (default 96) sun directions of a day's arc -- the ones
tools/raster_time.py's sun-hours row uses --, unit weights, curved.  Device times are events around the call, the device warm
(two untimed calls first), medians of --repeats.  Three rows, timed in the same process and alternated --rounds times:
  (a) irradiation   f3d_session_irradiation in its device form into a tensor that exists: energy alone, 4 bytes a sample out;
  (b) sun hours     f3d_session_raster in its device form on the same directions, count alone: every (sample, direction) pair
                    marches.  (a) marches a subset of these rays -- the pairs whose facet faces the sun;
  (c) by hand       what a caller does without the entry: f3d_session_raster for the K bit planes (device form), torch central
                    differences of the DEM for the gradient, then per direction the bits unpacked, the cosine and the weighted sum.
`b_spread_ms` is the spread between the repeated medians of (b) in this run: the margin within which (a) <= (b) is read.
(a) and (c) are compared; `max_abs_difference` is rounding (torch may fuse, the contract does not) and `count_mismatches` must be 0.

    python tools/irradiation_time.py [--dem 2048] [--directions 96] [--repeats 7] [--rounds 3]
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
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
        return statistics.median(values)

    out = {"config": f"rainier proxy {rows}x{cols}, {n} samples, {args.directions} directions, unit weights, curved, medians of {args.repeats}, "
                     f"{args.rounds} alternated rounds, warm, device events"}
    with TerrainSession(dem, args.width, args.height, cam, **kw) as s:
        sx, sz = np.float32(kw["spacing"][0]), np.float32(kw["spacing"][1])
        ox, oz = np.float32(-0.5 * (cols - 1.0) * float(sx)), np.float32(-0.5 * (rows - 1.0) * float(sz))
        bias = float(np.float32(s.SURFACE_BIAS))
        t = np.linspace(0.02, 0.98, args.directions)
        az, el = np.radians(90.0 + 180.0 * t), np.radians(2.0 + 48.0 * np.sin(np.pi * t))
        day = np.stack([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el), np.ones_like(t)], 1).astype(np.float32)
        d_day = torch.from_numpy(day).cuda()
        energy = torch.zeros(n, dtype=torch.float32, device="cuda")
        terms = torch.zeros(n, dtype=torch.int32, device="cuda")
        hours = torch.zeros(n, dtype=torch.int32, device="cuda")
        masks = torch.zeros((args.directions, words), dtype=torch.int64, device="cuda")

        def irradiation(count=None):
            q = _native.IrradiationDesc()
            q.struct_size = C.sizeof(_native.IrradiationDesc)
            q.flags = _native.IRRADIATION_CURVED | _native.IRRADIATION_DEVICE_POINTERS | _native.IRRADIATION_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, bias
            q.direction_count, q.directions = args.directions, d_day.data_ptr()
            q.energy = energy.data_ptr()
            q.count = count.data_ptr() if count is not None else None
            s._check(s._lib.f3d_session_irradiation(s._handle, C.byref(q), s._err, len(s._err)))

        def raster(m, c):
            q = _native.RasterDesc()
            q.struct_size = C.sizeof(_native.RasterDesc)
            q.mode = _native.RASTER_ALONG_DIRECTION
            q.flags = _native.RASTER_CURVED | _native.RASTER_DEVICE_POINTERS | _native.RASTER_NO_WAIT
            q.row0, q.col0, q.rows, q.cols, q.lift = 0, 0, rows, cols, bias
            q.target_count, q.targets = args.directions, d_day.data_ptr()
            q.masks = m.data_ptr() if m is not None else None
            q.count = c.data_ptr() if c is not None else None
            s._check(s._lib.f3d_session_raster(s._handle, C.byref(q), s._err, len(s._err)))

        # (c): the DEM as a tensor, the lattice in f64 rounded once -- the contract's planes
        heights = torch.from_numpy(dem.astype(np.float32)).cuda() * float(np.float32(kw["exaggeration"]))
        px = (torch.arange(cols, dtype=torch.float64, device="cuda") * float(sx) + float(ox)).float()
        pz = (torch.arange(rows, dtype=torch.float64, device="cuda") * float(sz) + float(oz)).float()
        bit = torch.arange(64, dtype=torch.int64, device="cuda")
        by_hand = torch.zeros(n, dtype=torch.float32, device="cuda")
        by_hand_terms = torch.zeros(n, dtype=torch.int32, device="cuda")

        def gradient():
            i, j = torch.arange(cols, device="cuda"), torch.arange(rows, device="cuda")
            iw, ie, jn, js = torch.clamp(i - 1, min=0), torch.clamp(i + 1, max=cols - 1), torch.clamp(j - 1, min=0), torch.clamp(j + 1, max=rows - 1)
            gx = (heights[:, ie] - heights[:, iw]) / (px[ie] - px[iw])[None, :]
            gz = (heights[js, :] - heights[jn, :]) / (pz[js] - pz[jn])[:, None]
            return gx.reshape(-1), gz.reshape(-1)

        def hand():
            raster(masks, None)
            gx, gz = gradient()
            q = (gx * gx + gz * gz) + 1.0
            by_hand.zero_()
            by_hand_terms.zero_()
            for k in range(args.directions):
                x, y, z, w = (float(v) for v in day[k])
                lit = (((masks[k].unsqueeze(-1) >> bit) & 1) != 0).reshape(-1)[:n]
                c = ((y - gx * x) - gz * z) / torch.sqrt(q * ((x * x + y * y) + z * z))
                on = lit & (c > 0.0)
                by_hand.add_(torch.where(on, w * c, torch.zeros_like(c)))
                by_hand_terms.add_(on.int())

        a, b, c = [], [], []
        for _ in range(args.rounds):  # alternated: the spread of (b) is the run's own noise
            b.append(device_ms(lambda: raster(None, hours)))
            a.append(device_ms(lambda: irradiation()))
            c.append(device_ms(hand))
        b.append(device_ms(lambda: raster(None, hours)))
        irradiation(terms)
        hand()
        torch.cuda.synchronize()
        out["a_irradiation_device_ms"] = {"median": statistics.median(a), "rounds": a}
        out["b_sun_hours_count_device_ms"] = {"median": statistics.median(b), "rounds": b}
        out["b_spread_ms"] = max(b) - min(b)
        out["c_by_hand_device_ms"] = {"median": statistics.median(c), "rounds": c}
        out["a_within_b_plus_spread"] = bool(statistics.median(a) <= statistics.median(b) + out["b_spread_ms"])
        out["mean_terms_lit"] = float(terms.float().mean())
        out["mean_hours_lit"] = float(hours.float().mean())
        out["count_mismatches"] = int((terms != by_hand_terms).sum())
        out["max_abs_difference"] = float((energy - by_hand).abs().max())
        out["mean_energy"] = float(energy.mean())
        # the share of (sample, direction) pairs whose facet faces the sun: the rays (a) marches of (b)'s
        gx, gz = gradient()
        facing = sum(float((((float(y) - gx * float(x)) - gz * float(z)) > 0.0).float().mean()) for x, y, z, _ in day) / args.directions
        out["marching_pairs_fraction"] = facing
        out["gpu_resource_bytes"] = s.info()["gpu_resource_bytes"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
