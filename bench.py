#!/usr/bin/env python
"""bench.py -- headline benchmark of the MI355X terrain path tracer.

Metric (BASELINE.json): Msamples/s = W*H*spp*frames / seconds of the accumulation loop, at
1920x1080, 256 spp (8 spp/frame x 32 frames), sun az 302 / el 24, on the synthetic
"rainier-proxy" 2048^2 DEM (the real Rainier DEM is a git-LFS object, unreachable here).
A "step" is one accumulation frame: one launch of the fused frame kernel over the whole
image (spp camera samples per pixel, each 1 primary + 1 sun-shadow + 1 IBL-occlusion
traversal, ReSTIR spatial+temporal reuse, accumulation, Welford).  Inputs (DEM tables,
state) are resident in HBM before the timed region.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, runs W untimed frames, times K frames and prints one JSON line
(`ms_per_step`: milliseconds per timed frame).  --dump-outputs DIR then writes the image of
the last timed frame (RGBA, albedo, normal, depth, hit mask) as finite float32 .npy files.
--full adds what the headline does not need: the golden scene's SSIM, further timed windows
and the kernel-timing window, the CPU baseline and the rooflines, the terrain-filling
camera, a real DEM when one is supplied, and BASELINE.json's other configurations.

N > 1 (launched by torch.distributed.run, one rank per GPU): the image is split into N
load-balanced row strips (measured before the timed region, forge3d_amd/distributed.py).
After every frame each strip PULLS the 4 edge rows of packed reservoirs of its two
neighbours itself, on the device, from their IPC-mapped memory over xGMI (peer halos: no
Python and no collective per frame; if the devices cannot map each other every rank
falls back to an RCCL send / recv pair per frame -- `config.peer_halos` says which ran).
RCCL carries the all-reduce of the variance record per window and the gather of the
RGBA8 / AOV strips to rank 0 at the end (strong scaling: the 1080p frame is fixed).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# State bytes per pixel-frame, S of SURVEY.md 8(d) -- ONE accounting, the same in DESIGN.md 4.1 / 6 and BASELINE.md 4:
#   1-lane kernel (head fused into k_frame): reservoir r16 + w16, accumulation r16 + w16, Welford m2 r4 + w4,
#   G-buffer r16 = 88 B.
#   Sample-lane form (the default): k_head reads reservoir 16 + G-buffer 16 and writes the parked history 16 + its 8-byte
#   record = 56 B, timed and priced apart; k_frame -- the kernel the roofline object is about -- reads the record 8 and the
#   parked history 16, writes the reservoir 16, accumulation r16 + w16, m2 r4 + w4 = 80 B.  (The frame as a whole: 136 B.)
STATE_BYTES_PER_PIXEL_FRAME = {False: 88, True: 80}
K_HEAD_STATE_BYTES = 56


def golden_scores(device: int):
    """SSIM / mean-abs of THIS build's render of the reference's locked golden scene against the reference's committed golden
    image (BASELINE.json's metric: "...; SSIM vs golden"; reference gate tests/test_hybrid_terrain_pt.py:858-859: SSIM >= 0.995,
    mean-abs <= 2.0).  The scene converges by the reference's Welford gate (256 frames of 1 spp at 256 x 256); tests/metrics.py
    restates the reference's SSIM (tests/_ssim.py).  The PNG is data the reference's own tests hold (tests/golden/)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import metrics

    from forge3d_amd import datasets, hybrid_render_terrain_reference, io

    dem, cam, kw = datasets.mini_dem_scene(np.load(ROOT / "tests" / "golden" / "mini_dem.npy"))
    t0 = time.perf_counter()
    out = hybrid_render_terrain_reference(dem, 256, 256, cam, **kw)
    seconds = time.perf_counter() - t0
    golden = io.png_to_numpy(ROOT / "tests" / "golden" / "mini_dem_reference.png")
    return {"ssim_vs_golden": metrics.ssim(out["rgba"][..., :3], golden[..., :3], data_range=255.0),
            "mean_abs_vs_golden": metrics.mean_abs(out["rgba"][..., :3], golden[..., :3]),
            "golden": {"scene": "reference golden scene: mini-DEM 128^2, 256x256, 1 spp/frame until the Welford gate fires",
                       "frames": int(out["frames"]), "gate": "SSIM >= 0.995 and mean-abs <= 2.0 (tests/test_hybrid_terrain_pt.py:858-859)",
                       "render_ms": round(seconds * 1e3, 2)}}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--dem", type=int, default=2048)
    ap.add_argument("--variant", type=int, default=int(os.environ.get("F3D_KERNEL_VARIANT", "0")))
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: the golden scene's SSIM, further timed windows and the "
                         "kernel-timing window, the CPU baseline and the rooflines, the terrain-filling camera, a real DEM, BASELINE.json's "
                         "other configurations.  Without it the run sets up, warms up, times --steps frames and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed frames, write the image the timed path produced in its last frame as DIR/<name>.npy "
                         "(float32, finite: rgba, albedo, normal, depth with 0 where the ray hit nothing, hit = 1 or 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline (and with it the rooflines)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="target CPU time of the cpu_baseline sample")
    ap.add_argument("--extra-windows", type=int, default=4, help="--full: further timed windows of --steps frames (spread report)")
    ap.add_argument("--no-recut", action="store_true", help="N > 1: keep the first cut of the strips whatever the warm-up frames cost each rank")
    ap.add_argument("--no-terrain-filling", action="store_true", help="--full: skip the second, terrain-filling camera")
    ap.add_argument("--no-configs", action="store_true", help="--full: skip the short timed windows of BASELINE.json's other configurations")
    ap.add_argument("--dem-path", default=None, help="--full: a real DEM (GeoTIFF / .npy) for an ADDITIONAL labelled run of the headline configuration; "
                                                     "default: $FORGE3D_REPO_ROOT/assets/tif/dem_rainier.tif when that exists (BASELINE.md section 3)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def kernel_source_hash() -> str:
    """SHA-256 over the frame kernel's sources (f3d_kernels.hip and every header it includes, transitively) plus the
    build flags: ties a PMC traffic figure under profiles/ to the device code it was measured on.  The host driver and
    the sources of the other rows (smoke, denoiser, LBVH ...) do not enter."""
    import hashlib
    import re

    csrc = ROOT / "forge3d_amd" / "csrc"
    todo, seen = ["f3d_kernels.hip"], set()
    while todo:
        name = todo.pop()
        if name in seen or not (csrc / name).exists():
            continue
        seen.add(name)
        todo += re.findall(r'#include\s+"([^"]+)"', (csrc / name).read_text())
    h = hashlib.sha256()
    for name in sorted(seen):
        h.update(name.encode())
        h.update((csrc / name).read_bytes())
    import __graft_entry__ as entry

    h.update(" ".join(entry.HIPCC_FLAGS + entry.KERNEL_FLAGS).encode())
    return h.hexdigest()[:16]


def terrain_filling_camera(dem, kw):
    """Second workload for the same DEM: a camera inside the footprint looking across the massif, so that nearly
    every pixel is terrain (the headline camera of BASELINE.json configs[1] sees ~60 % sky)."""
    spacing = kw["spacing"][0]
    span = (dem.shape[1] - 1) * spacing
    top = float(dem.max())
    return {"origin": (-0.30 * span, 0.62 * top, -0.34 * span), "look_at": (0.02 * span, 0.30 * top, 0.03 * span),
            "up": (0.0, 1.0, 0.0), "fov_y": 38.0, "exposure": 1.0}


def other_configs(dem, cam, kw, args, device):
    """Short timed windows of BASELINE.json's OTHER configurations, so that their rates are driver-observed and not
    only tool logs (round-2 verdict item 7).  Synthetic stand-ins as in BASELINE.md; the headline stays configs[1]."""
    import torch

    from forge3d_amd import atmosphere, datasets
    from forge3d_amd.session import TerrainSession

    out = {}

    def window(session, warm, frames, samples_per_frame):
        session.enqueue_frames(0, warm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        session.enqueue_frames(warm, frames, True)
        session.window_stats()
        dt = time.perf_counter() - t0
        return {"value": samples_per_frame * frames / dt / 1e6, "unit": "Msamples/s", "ms_per_step": dt / frames * 1e3, "steps": frames}

    # C1: the reference's locked mini-DEM scene at 512 x 512, 16 spp per frame (its CPU-snapshot configuration)
    try:
        mini = np.load(ROOT / "tests" / "golden" / "mini_dem.npy")
        d1, c1, k1 = datasets.mini_dem_scene(mini)
        k1 = dict(k1, spp=16, max_frames=20, min_frames=20, variance_threshold=1e30)
        with TerrainSession(d1, 512, 512, c1, device=device, memory_budget_bytes=8 << 30, frames_in_flight=0xFFFFFFFF, **k1) as s:
            r = window(s, 4, 16, 512 * 512 * 16)
            r["frames_in_flight"] = s.frames_in_flight()
        r["config"] = "BASELINE.json configs[0]: mini-DEM golden scene 128^2 DEM, 512x512, 16 spp/frame x 16 frames"
        out["C1"] = r
    except Exception as exc:  # noqa: BLE001
        out["C1"] = {"error": str(exc)[:200]}
    # C3: configs[1] + the AETHER aerial-perspective post at turbidity 2 (the post runs inside the resolve kernel)
    try:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (no bank directory on the GPU box: anchors baked, handle says so)
            handle = atmosphere.AtmosphereLutHandle.load_shipped(atmosphere.AtmosphereConfig(turbidity=2.0))
        k3 = dict(kw, max_frames=20, min_frames=20)
        with TerrainSession(dem, args.width, args.height, cam, device=device, memory_budget_bytes=8 << 30, kernel_variant=args.variant,
                            atmosphere=handle, **k3) as s:
            r = window(s, 4, 16, args.width * args.height * args.spp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img = s.resolve(20)
            r["resolve_with_post_and_readback_ms"] = (time.perf_counter() - t0) * 1e3
        r["hit_fraction"] = float(np.isfinite(img["depth"]).mean())
        r["lut_provenance"] = handle.provenance
        r["config"] = (f"BASELINE.json configs[2] stand-in: configs[1] workload + AETHER post (turbidity 2), {args.width}x{args.height}, "
                       f"{args.spp} spp/frame x 16 frames; GI (terrain in the PBR tracer) is not part of this number")
        out["C3"] = r
    except Exception as exc:  # noqa: BLE001
        out["C3"] = {"error": str(exc)[:200]}
    # C3 with GI: the DEM as the heightfield primitive of the PBR path tracer (multi-bounce) + the AETHER post on its radiance
    try:
        from forge3d_amd import offline

        k = dict(spacing=kw["spacing"], exaggeration=kw["exaggeration"], sun_azimuth_deg=kw["sun_azimuth_deg"], sun_elevation_deg=kw["sun_elevation_deg"],
                 sun_intensity=kw["sun_intensity"], atmosphere=handle, memory_budget_bytes=8 << 30)
        offline.render_terrain_gi(dem, args.width, args.height, cam, spp=8, **k)
        t0 = time.perf_counter()
        gi = offline.render_terrain_gi(dem, args.width, args.height, cam, spp=64, **k)
        wall = time.perf_counter() - t0
        out["C3_gi"] = {"value": args.width * args.height * 64 / gi["gi_seconds"] / 1e6, "unit": "Mpaths/s (multi-bounce paths, 1 per pixel-frame)",
                        "gi_loop_ms": gi["gi_seconds"] * 1e3, "wall_ms_incl_setup_post_readback": wall * 1e3,
                        "path_vertices_per_path": gi["path_vertices"] / (args.width * args.height * 64),
                        "config": f"BASELINE.json configs[2]: proxy DEM as heightfield primitive of the PBR path tracer (GI) + AETHER post, "
                                  f"{args.width}x{args.height}, 64 of 512 spp timed"}
    except Exception as exc:  # noqa: BLE001
        out["C3_gi"] = {"error": str(exc)[:200]}
    # C4 stand-in: 600 000 triangles (50 000 extruded boxes) on the proxy DEM at 4096 x 4096
    try:
        v, i = datasets.proxy_buildings(dem, kw["spacing"][0])
        k4 = dict(kw, max_frames=6, min_frames=6)
        with TerrainSession(dem, 4096, 4096, cam, device=device, memory_budget_bytes=16 << 30, mesh_vertices=v, mesh_indices=i, **k4) as s:
            r = window(s, 2, 4, 4096 * 4096 * args.spp)
        r["triangles"] = int(i.shape[0])
        r["config"] = f"BASELINE.json configs[3] stand-in: proxy DEM + 600 000 triangles, 4096x4096, {args.spp} spp/frame x 4 frames, 1 GPU"
        out["C4_standin"] = r
    except Exception as exc:  # noqa: BLE001
        out["C4_standin"] = {"error": str(exc)[:200]}
    # C5: the smoke sequence at 1080p: solver step -> ray-marcher -> composite over a terrain frame, 120 frames, everything
    # resident on the GPU (forge3d_amd.smoke.SmokeSequence: only the finished RGBA8 frames leave, through two pinned buffers)
    try:
        from forge3d_amd import smoke

        dims = (96, 64, 128)
        dom = smoke.SmokeDomain(dims)
        emitters = [smoke.SmokeEmitter(center=(48.0, 6.0, 40.0), radius=7.0, density_rate=9.0, temperature_rate=6.0, soot_rate=0.5,
                                       emission_rate=2.0, velocity=(0.0, 2.0, 0.6))]
        settings = smoke.SmokeStepSettings(dt=0.2, turbulence_strength=0.5, turbulence_seed=7, wind=(0.3, 0.0, 1.0), buoyancy=1.1)
        view = dict(camera_pos=(48.0, 70.0, -120.0), target=(48.0, 28.0, 64.0), up=(0.0, 1.0, 0.0), fovy_deg=40.0)
        yy, xx = np.mgrid[0:args.height, 0:args.width]
        terrain = np.stack([(xx * 255 // max(1, args.width - 1)), (yy * 255 // max(1, args.height - 1)), np.full_like(xx, 96),
                            np.full_like(xx, 255)], axis=-1).astype(np.uint8)
        seq = smoke.SmokeSequence(dom, terrain, **view)
        for _ in seq.frames(40, settings, emitters):  # a developed plume (untimed)
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames5, last = 120, None
        for frame in seq.frames(frames5, settings, emitters):  # (untimed calls: the host enqueues ahead of the device)
            last = frame
        wall = (time.perf_counter() - t0) * 1e3 / frames5
        last = np.array(last)
        # the kernels' shares from a second, short pass in which every call records and waits for its device time
        timed, kernel = 24, {"solver_step": 0.0, "march": 0.0, "composite": 0.0}
        for _ in seq.frames(timed, settings, emitters, timing=True):
            for key in kernel:
                kernel[key] += seq.kernel_seconds[key]
        kernel_ms = {key: v * 1e3 / timed for key, v in kernel.items()}
        list_stats = seq.stats()  # what the sequence holds on the device, and how full the marcher's deferred list was (the timing pass above ran the serial schedule)
        out["C5"] = {"value": wall, "unit": "ms/frame (solver step + march + composite, state and images resident on the GPU; RGBA8 frames read back)",
                     "frames": frames5, "frames_per_s": 1e3 / wall, "kernel_ms": kernel_ms,
                     "kernel_ms_note": "device time by kernel group, from 24 further frames with per-call timing, one call after the other "
                                       "(in the 120 timed frames the solver's step runs beside the previous frame's march: the sum exceeds the wall)",
                     "kernel_sum_over_wall": sum(kernel_ms.values()) / wall,
                     "smoke_pixels": int(np.count_nonzero(np.any(last[..., :3] != terrain[..., :3], axis=-1))),
                     "sequence_scratch": list_stats,
                     "config": f"BASELINE.json configs[4] stand-in, SMOKE ONLY (the terrain frame under it is a fixed synthetic gradient: no terrain sample is in this number, "
                               f"see C5_with_terrain): {frames5} frames of the smoke sequence at {args.width}x{args.height}, 96x64x128 domain, "
                               "one emitter, frames 41..160 of the run, 1 GPU; solver: one launch per phase, a step ahead of the marcher on a stream of its own; "
                               "marcher: rays listed, self-shadow marches as a launch of their own, list shaded"}
        # C5 as BASELINE.json words it -- "1920x1080 at 64 spp x 120 frames": every sequence frame gets its own 64-spp terrain
        # render (8 accumulation frames of 8 spp in a fresh TerrainSession, the sun's azimuth advancing with the frame so that no
        # frame can reuse another's image) resolved on the device into the image the smoke is laid over.  Round 5's number
        # (above) composites over a fixed synthetic gradient and contains no terrain sample.
        try:
            seq2 = smoke.SmokeSequence(smoke.SmokeDomain(dims), terrain, **view)
            for _ in seq2.frames(40, settings, emitters):
                pass
            split = {"session_create": 0.0, "enqueue_and_resolve": 0.0, "session_close": 0.0}

            held = {"prev": None}  # the session of the frame before: closed only once the next one exists

            def terrain_frame(i, base, stream):
                # The frame's session is CREATED while the device still renders the frame before (its host work -- DEM fingerprint,
                # uniforms, allocation: 1.5 ms -- hides behind those kernels), then the session before is closed (a wait for work that
                # is done or nearly), then this frame's render is enqueued behind it on the same stream.  Round 6's first form closed
                # a frame's session right after enqueueing it: the host waited out every render before it began the next session.
                k = dict(kw, sun_azimuth_deg=float(kw["sun_azimuth_deg"]) + 0.25 * (i + 1), max_frames=8, min_frames=8)
                t = time.perf_counter()
                s = TerrainSession(dem, args.width, args.height, cam, device=device, stream=stream.cuda_stream, memory_budget_bytes=8 << 30,
                                   kernel_variant=args.variant, **k)
                t1 = time.perf_counter()
                if held["prev"] is not None:
                    held["prev"].close()  # (waits for that session's work: its buffers go back to the library's pool)
                t2 = time.perf_counter()
                s.enqueue_frames(0, 8)
                s.resolve_device(8, d_rgba=base.data_ptr())
                held["prev"] = s
                t3 = time.perf_counter()
                split["session_create"] += t1 - t
                split["session_close"] += t2 - t1
                split["enqueue_and_resolve"] += t3 - t2

            for _ in seq2.frames(3, settings, emitters, base_provider=terrain_frame):  # (first sessions of this size: pool and scene cache fill)
                pass
            for key in split:
                split[key] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last2 = None
            for frame in seq2.frames(frames5, settings, emitters, base_provider=terrain_frame):
                last2 = frame
            wall2 = (time.perf_counter() - t0) * 1e3 / frames5
            last2 = np.array(last2)
            if held["prev"] is not None:
                held["prev"].close()
                held["prev"] = None
            out["C5_with_terrain"] = {
                "value": wall2, "unit": "ms/frame (64-spp terrain render + solver step + march + composite; RGBA8 frames read back)",
                "frames": frames5, "frames_per_s": 1e3 / wall2, "terrain_spp_per_frame": 64,
                "terrain_msamples_per_s": args.width * args.height * 64 / (wall2 * 1e-3) / 1e6,
                "host_ms_per_frame": {key: round(v * 1e3 / frames5, 3) for key, v in split.items()},
                "host_ms_note": "wall time of the host calls per frame; a frame's session is created while the device renders the frame before, then the "
                                "session before is closed (session_close waits for ITS terrain kernels -- 8 x k_head + k_frame, resolve -- so most of the "
                                "terrain render's device time shows up there), then this frame's render is enqueued",
                "smoke_only_ms_per_frame": wall, "terrain_share_ms_per_frame": wall2 - wall,
                "terrain_pixels": int(np.count_nonzero(np.any(last2[..., :3] != terrain[..., :3], axis=-1))),
                "config": f"BASELINE.json configs[4] as worded: {frames5} frames at {args.width}x{args.height}, each a 64-spp terrain render of the proxy DEM "
                          "(8 accumulation frames x 8 spp, sun azimuth +0.25 deg per frame, fresh session per frame, created while the frame before renders: tables from the scene cache) under the "
                          "smoke sequence of configs.C5, 1 GPU"}
        except Exception as exc:  # noqa: BLE001
            out["C5_with_terrain"] = {"error": str(exc)[:200]}
    except Exception as exc:  # noqa: BLE001
        out["C5"] = {"error": str(exc)[:200]}
    return out


def cpu_baseline(dem, cam, kw, args, world=1):
    """Time the CPU oracle (test infrastructure, used here ONLY as the reported baseline) on a
    bounded sample of the same workload: same DEM/camera/sun/spp, resolution and frame count
    sized for ~args.cpu_seconds of CPU work; also returns the per-sample traversal
    counts that define the algorithmic bytes.  With world > 1 (the baseline is
    an N = 1 figure) only the two-frame counting run is made, for the roofline of the strip kernel."""
    from oracle import oracle

    oracle.build()
    # torch.distributed.run exports OMP_NUM_THREADS=1 to its workers: give the oracle its share of the host
    if world > 1 or os.environ.get("OMP_NUM_THREADS") == "1":
        oracle.set_num_threads(max(1, (os.cpu_count() or 1) // max(1, world)))
    cores = oracle.num_threads()
    k = dict(kw, spp=args.spp, max_frames=2, min_frames=2, variance_threshold=1e30)
    w, h = 240, 135
    probe = oracle.render(dem, w, h, cam, **k)
    rate = probe["n_samples"] / max(probe["loop_seconds"], 1e-9)
    budget = (2.0 if world > 1 else args.cpu_seconds) * rate  # samples the host can trace in the target time
    scale = min(args.width / w, max(1.0, (budget / probe["n_samples"]) ** 0.5))
    w2, h2 = min(args.width, int(w * scale) // 8 * 8), min(args.height, int(h * scale) // 8 * 8)
    out = oracle.render(dem, w2, h2, cam, **k)  # 2 frames at the sample's resolution: the real rate
    # the per-sample traversal counts of the roofline always come from these two frames (a fixed definition,
    # independent of how fast the host is)
    counts = {key: out[key] / out["n_samples"] for key in ("n_node", "n_leaf", "n_hit")}
    if world > 1:
        return None, counts
    frames = int(min(32, args.cpu_seconds * out["n_samples"] / max(out["loop_seconds"], 1e-9) // (w2 * h2 * args.spp)))
    if frames >= 3:
        k.update(max_frames=frames, min_frames=frames)
        out = oracle.render(dem, w2, h2, cam, **k)
    else:
        frames = 2
    n = out["n_samples"]
    return {
        "value": n / out["loop_seconds"] / 1e6, "unit": "Msamples/s", "cores": cores, "kind": "port",
        "sample": f"CPU oracle (C, OpenMP), same DEM/camera/sun, {w2}x{h2}, {args.spp} spp x {frames} frames "
                  f"= {n / 1e6:.2f} Msamples in {out['loop_seconds']:.1f} s",
    }, counts


DUMP_BYTES = 64_000_000  # --dump-outputs writes at most this much
DUMP_SEED = 20261016


def dump_outputs(directory, image) -> None:
    """--dump-outputs: the arrays a caller of the renderer receives (resolve: RGBA8, albedo, normal, depth) as float32 .npy
    files, every value finite.  The renderer marks a pixel whose camera ray hits nothing (sky) with a NaN depth; the dump
    writes depth 0 there and says which pixels hit in `hit` (1.0 terrain, 0.0 sky) -- a hit's depth is a positive distance.
    When the whole image does not fit in DUMP_BYTES, every array keeps the same fixed, seeded sample of pixels in raster
    order, shape (pixels, channels); otherwise the arrays keep their image shape."""
    arrays = {key: np.asarray(image[key]).astype(np.float32) for key in ("rgba", "albedo", "normal", "depth")}
    hit = ~np.isnan(arrays["depth"])
    arrays["depth"] = np.where(hit, arrays["depth"], np.float32(0.0))
    arrays["hit"] = hit.astype(np.float32)
    bad = [key for key, a in arrays.items() if not np.isfinite(a).all()]
    if bad:  # anything else that is not finite is a defect of the render, not a value to write
        raise ValueError(f"--dump-outputs: non-finite values in {', '.join(bad)} of the last timed frame")
    h, w = arrays["depth"].shape[:2]
    pixel_bytes = sum(a[0, 0].nbytes for a in arrays.values())
    if h * w * pixel_bytes > DUMP_BYTES:
        keep = np.sort(np.random.default_rng(DUMP_SEED).choice(h * w, DUMP_BYTES // pixel_bytes, replace=False))
        arrays = {key: a.reshape(h * w, -1)[keep] for key, a in arrays.items()}
    out = Path(directory)
    out.mkdir(parents=True, exist_ok=True)
    for key, a in arrays.items():
        np.save(out / f"{key}.npy", a)


def pmc_kernel_ms(issue: dict):
    """Average duration of the profiled launches behind an `issue` block (tools/gpu_profile.sh stores it), or None."""
    v = issue.get("kernel_ms_profiled")
    return float(v) if v else None


def device_identity(torch, index: int) -> dict:
    """What tells two devices apart in the line: index, name and whichever of uuid / PCI ids this torch build exposes."""
    props = torch.cuda.get_device_properties(index)
    ident = {"index": int(index), "name": str(props.name)}
    for key in ("uuid", "pci_bus_id", "pci_device_id", "pci_domain_id", "gcnArchName"):
        value = getattr(props, key, None)
        if value is not None:
            ident[key] = str(value)
    return ident


def recut_after_warmup(r, busy_ms, make_renderer, threshold=1.05):
    """ONE re-cut of the strips from what the warm-up frames cost each rank on the strips it will be timed on (VERDICT r5
    next 3b: ROW_COST_FLOOR was calibrated on one GPU and one scene).  busy_ms: every rank's time for the warm-up minus the
    time its halo pulls stood waiting for a neighbour (the same list on every rank, so every rank decides the same).
    Returns (renderer, report); the old renderer stays when the strips are balanced, the new cut equals the old one, or
    the new renderer cannot be built (then every rank raises inside its constructor's agreement and keeps the old one)."""
    from forge3d_amd.distributed import HALO_ROWS, partition_rows, rebalance

    mean = float(np.mean(busy_ms))
    report = {"busy_ms_per_rank": [round(x, 4) for x in busy_ms], "max_over_mean": round(max(busy_ms) / mean, 4) if mean > 0 else None,
              "threshold": threshold, "recut": False}
    if not (mean > 0.0 and all(np.isfinite(busy_ms)) and min(busy_ms) > 0.0) or max(busy_ms) / mean <= threshold:
        return r, report
    density = np.asarray(getattr(r, "cost_density", np.ones(r.height)), np.float64)
    bounds = partition_rows(rebalance(density, r.bounds, busy_ms), r.world, HALO_ROWS)
    report["bounds_before"], report["bounds_after"] = list(r.bounds), list(bounds)
    if bounds == list(r.bounds):
        return r, report
    try:
        new = make_renderer(bounds)
    except Exception as exc:  # noqa: BLE001 -- raised on every rank (StripRenderer._agree): everybody keeps the old strips
        report["failed"] = str(exc)[:200]
        return r, report
    r.close()
    report["recut"] = True
    return new, report


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback)")
    if os.environ.get("F3D_DIST_BACKEND") == "gloo":  # rehearsal: all ranks share the one GPU of a test box
        local_rank = 0
    torch.cuda.set_device(local_rank)
    from forge3d_amd import datasets
    from forge3d_amd.distributed import HALO_ROWS, StripRenderer, init_process_group

    init_process_group(world, rank)
    dem, cam, kw = datasets.rainier_proxy_scene(args.dem)
    kw = dict(kw, spp=args.spp, variance_threshold=1e30)

    # a plain run times one window and accumulates nothing after it; --full adds the further windows and the kernel-timing one
    windows = 1 + max(0, args.extra_windows) if args.full else 1
    total_frames = args.warmup + args.steps * (max(windows, 2) if args.full else 1)  # (one window more when the kernel-timing window is an extra one)
    kw = dict(kw, max_frames=max(total_frames, 2), min_frames=max(total_frames, 2))
    if True:  # (every rank) a throw-away session of another DEM first: module load and allocator start-up are not set-up of THIS render
        from forge3d_amd.session import TerrainSession

        # (large enough to go through the staged upload: the first asynchronous host-to-device copy of a process costs 7 ms)
        warm = np.zeros((768, 768), np.float32)
        warm[::3, ::5] = 1.0
        with TerrainSession(warm, 64, 64, cam, device=local_rank, **dict(kw, max_frames=2, min_frames=2)) as ws:
            ws.enqueue_frames(0, 2)
        torch.zeros(4, dtype=torch.int32, device=f"cuda:{local_rank}")  # (torch's own allocator and stream start up with its first device tensor: 15-20 ms on some boxes)
        torch.cuda.synchronize()
    golden_report = None
    if rank == 0 and args.full:
        # the reference's golden scene, rendered and scored for the line's "SSIM vs golden" -- in front of the set-up and the timed
        # windows rather than behind them: it is 256 frames of device work the bench does anyway, and a device that has just
        # done it runs the first timed window at the clocks of the later ones (it used to be 1.5 % slower than windows 2-5)
        try:
            golden_report = golden_scores(local_rank)
        except Exception as exc:  # noqa: BLE001 -- a report, never a reason to lose the line
            golden_report = {"ssim_vs_golden": None, "golden": {"error": str(exc)[:200]}}
    if world > 1:  # every rank has started up, and the process group has made its connections (once per process, not per render)
        import torch.distributed as dist

        comm = "cpu" if dist.get_backend() == "gloo" else f"cuda:{local_rank}"
        warm_box = torch.zeros(8, dtype=torch.float64, device=comm)
        dist.all_reduce(warm_box)  # (each kind of collective the set-up uses, once: their first use builds the backend's channels)
        dist.broadcast(warm_box, src=0)
        dist.all_gather([torch.empty_like(warm_box) for _ in range(world)], warm_box)
        dist.barrier()
        # what the process group IS, from the group itself (not from the environment that asked for it), and which device
        # every rank really renders on: N distinct devices must be visible in the line
        identities = [None] * world
        dist.all_gather_object(identities, {"rank": rank, "host": os.uname().nodename, "pid": os.getpid(), **device_identity(torch, local_rank)})
        group = {"rccl_ranks": int(dist.get_world_size()), "dist_backend": str(dist.get_backend()), "rank_devices": identities,
                 "distinct_devices": len({(d.get("host"), d.get("uuid") or d.get("pci_bus_id") or d.get("index")) for d in identities})}
    else:
        group = {"rank_devices": [{"rank": 0, **device_identity(torch, local_rank)}]}
    torch.cuda.synchronize()
    t_setup = time.perf_counter()
    def make_renderer(row_bounds=None):
        return StripRenderer(dem, args.width, args.height, cam, rank=rank, world=world, device=local_rank, row_bounds=row_bounds,
                             kernel_variant=args.variant, memory_budget_bytes=8 << 30, **kw)

    r = make_renderer()
    torch.cuda.synchronize()
    # once per render, outside the timed region: DEM upload, min-max tables, G-buffer pass, ray certificates
    setup_ms = (time.perf_counter() - t_setup) * 1e3
    setup_phases = r.session.setup_ms() if hasattr(r.session, "setup_ms") else {}
    setup_trace, first_balance = dict(getattr(r, "setup_trace", {})), list(r.balance_log)
    # warmup (untimed) ---------------------------------------------------------------
    recut = None
    if world > 1 and args.warmup > 0 and not args.no_recut:
        # the warm-up runs on the strips that will be timed: what it cost each rank decides whether they are cut once more
        if r.peer_halos:
            r.session.halo_stats(reset=True)
        r.barrier()
        torch.cuda.synchronize()
        t_warm = time.perf_counter()
        r.run_frames(0, args.warmup)
        torch.cuda.synchronize()
        warm_ms = (time.perf_counter() - t_warm) * 1e3
        if r.peer_halos:  # a strip that waits for its neighbours is not a slow strip
            warm_ms = max(warm_ms - sum(r.session.halo_stats()["wait_ms"]), 1e-3)
            busy = r._gather_floats(warm_ms)
            t_recut = time.perf_counter()
            r, recut = recut_after_warmup(r, busy, make_renderer)
            recut["ms"] = round((time.perf_counter() - t_recut) * 1e3, 2)
            if recut["recut"]:
                r.run_frames(0, args.warmup)  # the new strips' own warm-up (the accumulation starts again at frame 0)
        else:
            recut = {"recut": False, "why": "classic halo exchange: a rank's waits are inside the collectives and cannot be told from its work"}
    else:
        r.run_frames(0, args.warmup)
    if r.peer_halos:
        r.session.halo_stats(reset=True)  # the warm-up's waits (first launches, code loads) are not the loop's
    r.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r.run_frames(args.warmup, args.steps)
    torch.cuda.synchronize()
    r.barrier()
    elapsed = time.perf_counter() - t0
    halo = r.session.halo_stats() if r.peer_halos else None
    rank_ms = r._gather_floats(elapsed / args.steps * 1e3) if world > 1 else [elapsed / args.steps * 1e3]
    halo_wait_ms = r._gather_floats(sum(halo["wait_ms"]) / args.steps) if (world > 1 and halo) else None
    halo_longest_ms = r._gather_floats(halo["longest_wait_ms"]) if (world > 1 and halo) else None
    elapsed = r.max_over_ranks(elapsed)
    # what the timed path computed in its last frame, as its caller receives it (rank 0; every rank takes part in the gather)
    last_image = r.gather_image(args.warmup + args.steps) if (args.dump_outputs or not args.full) else None
    # --full: further windows of the same K frames (the accumulation simply continues): the spread of the measurement.  The
    # frame kernel is timed (two hip events around every launch) in the LAST of them, or -- with --extra-windows 0 --
    # in a window of its own after the timed region: the headline window runs without the events.
    window_ms = [elapsed / args.steps * 1e3]
    kernel_ms, launches = 0.0, 0
    for wi in range(1, windows + (1 if windows == 1 else 0)) if args.full else ():
        timed_kernels = wi == max(1, windows - 1)
        r.barrier()
        torch.cuda.synchronize()
        if timed_kernels:
            r.session.kernel_timing(True)
        t1 = time.perf_counter()
        r.run_frames(args.warmup + wi * args.steps, args.steps)
        torch.cuda.synchronize()
        r.barrier()
        dt = r.max_over_ranks(time.perf_counter() - t1) / args.steps * 1e3
        if timed_kernels:
            kernel_ms, launches = r.session.kernel_timing(False)
            kernel_ms = r.max_over_ranks(kernel_ms)
        if wi < windows:
            window_ms.append(dt)
    # final composition (untimed, but exercised): gather strips to rank 0
    image = r.gather_image(total_frames) if args.full else last_image
    halo_bytes = 0 if world == 1 else HALO_ROWS * args.width * 16 * ((1 if rank > 0 else 0) + (1 if rank < world - 1 else 0))
    warnings = []
    if world > 1:
        import torch.distributed as dist

        reasons = [None] * world
        dist.all_gather_object(reasons, getattr(r, "peer_halo_failure", None))
        if not r.peer_halos:  # LOUD: the line is then a measurement of the fall-back, not of the design
            warnings.append("PEER HALOS OFF: the strips exchanged their halo rows through an RCCL send / recv pair per frame "
                            "(Python and a collective per frame) instead of pulling them on the device; reasons by rank: "
                            + json.dumps(reasons))
        if group.get("distinct_devices") != world:
            warnings.append(f"{world} ranks on {group.get('distinct_devices')} distinct device(s): "
                            + ("a one-GPU rehearsal (F3D_DIST_BACKEND=gloo), NOT a scaling measurement" if os.environ.get("F3D_DIST_BACKEND") == "gloo"
                               else "ranks share devices"))
        if getattr(r, "cost_probe_failed_ranks", None):
            warnings.append(f"cost-map probe failed on ranks {r.cost_probe_failed_ranks}: their rows were cut at the mean cost")
        for w in warnings:
            if rank == 0:
                print("bench.py WARNING:", w, file=sys.stderr, flush=True)

    if rank == 0:
        samples_per_step = args.width * args.height * args.spp
        value = samples_per_step * args.steps / elapsed / 1e6
        result = {
            # BASELINE.json's metric, with the resolution and sample count of THIS run written out (the steady-state rate per
            # accumulation frame does not depend on how many frames the run accumulates: windows_ms_per_step)
            "metric": f"Msamples/s (W*H*spp/s) at {args.width}x{args.height}, {args.spp * args.steps} spp "
                      f"({args.spp} spp/frame x {args.steps} frames timed); SSIM vs golden", "value": value, "unit": "Msamples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            # the timed region above is window 0; the others repeat it on the continuing accumulation
            "windows_ms_per_step": [round(x, 4) for x in window_ms],
            "median_window_ms_per_step": float(np.median(window_ms)),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
            **({"warnings": warnings} if warnings else {}),
            "data": "synthetic (rainier-proxy 2048^2 DEM, seed 20260926; real Rainier DEM is git-LFS)",
            "config": {
                "workload": f"BASELINE.json configs[1]: rainier-proxy DEM {args.dem}x{args.dem}, "
                            f"{args.width}x{args.height}, {args.spp} spp/frame x {args.steps} frames "
                            f"= {args.spp * args.steps} spp, sun az302/el24, orbit phi28/theta49 fov42",
                "parallelism": "1 GPU" if world == 1 else (
                    f"{world} load-balanced row strips; halos: " + ("pulled by the strips from IPC-mapped peer memory (device-side, no collective per frame)"
                                                                   if r.peer_halos else "RCCL send / recv pair per frame")
                    + "; RCCL all-reduce per window + gather of the strips"),
                **({"peer_halos": bool(r.peer_halos)} if world > 1 else {}),
                "kernel_variant": args.variant,
                "frames_in_flight": r.session.frames_in_flight(),
                "setup_ms_once_per_render": round(setup_ms, 3),
                # f3d_session_setup_ms: host wall time of the session's creation by phase (validate = one pass over the DEM: finiteness
                # + the scene cache's key; upload + tables are 0 for a cached DEM; alloc = per-pixel state + clears; passes = ENQUEUEING
                # the G-buffer / certificate kernels); device_passes = until those kernels have run (G-buffer, primary-start and
                # sun-cylinder certificates: about 1.1 ms at 1080p, paid back in about 3 frames); the rest of setup_ms_once_per_render is
                # this script's Python around the session (balancing probes and peer-halo set-up when N > 1)
                "setup_ms": {**{k: round(v, 3) for k, v in setup_phases.items()},
                             "device_passes_and_python": round(setup_ms - setup_phases.get("total", 0.0), 3)},
                "setup_note": "session creation outside the timed region, for a DEM this process has not seen: DEM fingerprint, staged upload, "
                              "min-max tables, state allocation + clears, G-buffer pass, ray certificates",
                **({"setup_trace_ms_rank0": {k: round(v, 2) for k, v in setup_trace.items()}, "strip_row_bounds": r.bounds, "strip_probe_ms": r.balance_log[-1]["ms"] if r.balance_log else None,
                    "strip_cut": (first_balance[-1].get("from") if first_balance else "equal rows"),
                    "cost_probe_failed_ranks": list(getattr(r, "cost_probe_failed_ranks", [])),
                    # one re-cut from what the warm-up frames cost each rank on the strips of the first cut (busy = wall - halo waits)
                    "recut_after_warmup": recut,
                    **group, "rank_ms_per_step": [round(x, 4) for x in rank_ms], "halo_bytes_per_frame_rank0": halo_bytes,
                    # device time each rank's pulls stood waiting for its neighbours' frame counters, per frame (peer halos only),
                    # and the longest single wait: what the first real multi-GPU run has to show
                    "halo_wait_ms_per_frame": [round(x, 4) for x in halo_wait_ms] if halo_wait_ms else None,
                    "halo_longest_wait_ms": [round(x, 4) for x in halo_longest_ms] if halo_longest_ms else None,
                    } if world > 1 else {"rank_devices": group["rank_devices"]}),
            },
        }
        counts = None
        if args.full and not args.no_cpu_baseline:
            try:
                baseline, counts = cpu_baseline(dem, cam, kw, args, world)
                if baseline is not None:  # reported at N = 1 only
                    result["cpu_baseline"] = baseline
            except Exception as exc:  # the baseline is a report, never a reason to lose the GPU number
                result["cpu_baseline"] = {"value": None, "unit": "Msamples/s", "cores": 0, "kind": "port",
                                          "sample": f"failed: {exc}"}
        if counts is not None:
            # algorithmic bytes per sample: S/k + 8 n_node + 16 n_leaf + 16 n_hit
            lanes = r.session.sample_lanes()
            b_alg = (STATE_BYTES_PER_PIXEL_FRAME[lanes > 1] / args.spp + 8.0 * counts["n_node"] + 16.0 * counts["n_leaf"]
                     + 16.0 * counts["n_hit"])
            per_launch = b_alg * samples_per_step / world
            # strips launch the frame kernel twice per frame (edge rows, interior): price the frame, not the launch
            frame_kernel_ms = kernel_ms * launches / max(1, args.steps)
            achieved = per_launch / (frame_kernel_ms * 1e-3) / 1e9
            # HBM bytes per launch from the rocprofv3 PMC passes of the SAME command (committed
            # under profiles/; bench.py cannot run the profiler itself): only quoted when the
            # run matches the profiled configuration.
            traffic, traffic_note = None, "no PMC profile of these kernel sources under profiles/"
            issue = None
            try:
                # the newest profile of THESE kernel sources wins (rNN_pmc_traffic.json, written by tools/gpu_profile.sh)
                for path in sorted((ROOT / "profiles").glob("r*_pmc_traffic.json"), reverse=True):
                    pmc = json.loads(path.read_text())
                    if pmc.get("kernel_source_hash") != kernel_source_hash():
                        traffic_note = f"profiles/{path.name} was measured on other kernel sources: not quoted"
                        continue
                    if (world == 1 and (args.width, args.height, args.spp, args.dem) == (1920, 1080, 8, 2048)
                            and pmc.get("sample_lanes", 1) == lanes):
                        traffic = pmc["hbm_bytes_per_launch"]
                        traffic_note = f"rocprofv3 PMC passes of this command on these kernel sources (profiles/{path.name})"
                        issue = dict(pmc.get("issue") or {}, profile=f"profiles/{path.name}") if pmc.get("issue") else None
                    break
            except Exception:
                pass
            result["roofline"] = {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_note": traffic_note,
                "kernel": "k_trace" if r.session.frames_in_flight() else "k_frame",
                "kernel_ms": frame_kernel_ms, "launches": launches, "bytes_per_sample": b_alg, "sample_lanes": lanes,
                "per_sample_counts": counts,
            }
            if issue:
                # The roof this kernel is actually under (HBM traffic is 0.38x the algorithmic bytes and a fraction
                # of the peak; the march is instruction-bound): vector instructions issued per second against what 1 024 SIMDs
                # can issue -- one wave instruction every 2 cycles (MI355X_MICROARCH.md; this kernel's own calibration run,
                # profiles/r03_valu_calib.log, measured 2.4) at the clock the profiled launches ran at.  achieved is the profile's
                # instruction count over THIS run's kernel time.
                instr = float(issue["valu_wave_instructions_per_launch"])
                cycles = float(issue["gpu_cycles_per_launch"])
                clock_hz = cycles / (float(pmc_kernel_ms(issue)) * 1e-3) if pmc_kernel_ms(issue) else None
                peak = 1024.0 * (clock_hz or 2.4e9) / 2.0
                achieved_issue = instr / (frame_kernel_ms * 1e-3)
                result["roofline_issue"] = {
                    "bound": "valu_issue", "achieved": achieved_issue / 1e12, "peak": peak / 1e12, "unit": "T wave-instructions/s",
                    "frac": achieved_issue / peak, "frac_counters_only": instr * 2.0 / (1024.0 * cycles),
                    "lane_utilisation": issue["lane_utilisation"], "useful_frac": achieved_issue / peak * issue["lane_utilisation"],
                    "wait_fraction_of_wave_cycles": issue["wait_fraction_of_wave_cycles"], "salu_per_valu": issue["salu_per_valu"],
                    "cycles_per_issue": 2.0, "clock_ghz": (clock_hz or 2.4e9) / 1e9, "simds": 1024,
                    "valu_wave_instructions_per_launch": instr, "kernel": "k_frame", "profile": issue["profile"],
                    "note": "useful_frac = frac x lane_utilisation: the share of the chip's lane-cycles that do this kernel's arithmetic",
                }
        if image is not None:
            result["config"]["image_mean_rgb"] = [float(x) for x in image["rgba"][..., :3].mean((0, 1))]
            # what the samples were: the headline camera looks past the mountain (mostly sky)
            hit = float(np.isfinite(image["depth"]).mean())
            result["hit_fraction"] = hit  # centre rays that hit terrain
            result["shaded_msamples_per_s"] = value * hit  # samples that were shaded (sun + sky ray each)
            result["grays_per_s"] = value * 1e6 * (1.0 + 2.0 * hit) / 1e9  # primary + 2 occlusion rays per shaded sample
        result["kernel_source_hash"] = kernel_source_hash()
    r.close()
    if rank == 0 and golden_report is not None:
        result.update(golden_report)
    if args.full and rank == 0 and world == 1 and not args.no_terrain_filling:
        # the same DEM from inside the footprint: (nearly) every sample is shaded -- a harder number than the headline
        cam2 = terrain_filling_camera(dem, kw)
        frames2 = 4 + 16
        r2 = StripRenderer(dem, args.width, args.height, cam2, rank=0, world=1, device=local_rank, kernel_variant=args.variant,
                           memory_budget_bytes=8 << 30, **dict(kw, max_frames=frames2, min_frames=frames2))
        r2.run_frames(0, 4)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r2.run_frames(4, 16)
        torch.cuda.synchronize()
        dt2 = time.perf_counter() - t2
        img2 = r2.gather_image(frames2)
        r2.close()
        rate2 = args.width * args.height * args.spp * 16 / dt2 / 1e6
        hit2 = float(np.isfinite(img2["depth"]).mean())
        result["config_terrain_filling"] = {
            "value": rate2, "unit": "Msamples/s", "ms_per_step": dt2 / 16 * 1e3, "steps": 16, "hit_fraction": hit2,
            "shaded_msamples_per_s": rate2 * hit2, "grays_per_s": rate2 * 1e6 * (1.0 + 2.0 * hit2) / 1e9,
            "camera": {k: [float(x) for x in v] if isinstance(v, tuple) else v for k, v in cam2.items()},
        }
    if args.full and rank == 0 and world == 1:
        # "if a real dem_rainier.tif is supplied via FORGE3D_REPO_ROOT, S2 is run on it as well and
        # labelled" (reference python/forge3d/datasets.py:53-61, :312 fetch_dem('rainier')).  The headline stays the proxy.
        real_path = args.dem_path
        if real_path is None:
            try:
                real_path = str(datasets.fetch_dem("rainier"))
            except (FileNotFoundError, KeyError):
                real_path = None
        if real_path:
            try:
                rdem, rcam, rkw, what = datasets.real_dem_scene(real_path)
                frames_r = args.warmup + args.steps
                rr = StripRenderer(rdem, args.width, args.height, rcam, rank=0, world=1, device=local_rank, kernel_variant=args.variant, memory_budget_bytes=16 << 30,
                                   **dict(rkw, spp=args.spp, variance_threshold=1e30, max_frames=frames_r, min_frames=frames_r))
                rr.run_frames(0, args.warmup)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                rr.run_frames(args.warmup, args.steps)
                torch.cuda.synchronize()
                dt3 = time.perf_counter() - t3
                img3 = rr.gather_image(frames_r)
                rr.close()
                result["config_real_dem"] = {"value": args.width * args.height * args.spp * args.steps / dt3 / 1e6, "unit": "Msamples/s",
                                             "ms_per_step": dt3 / args.steps * 1e3, "steps": args.steps, "data": "real: " + what,
                                             "hit_fraction": float(np.isfinite(img3["depth"]).mean()),
                                             "image_mean_rgb": [float(x) for x in img3["rgba"][..., :3].mean((0, 1))]}
            except Exception as exc:  # noqa: BLE001 -- an unreadable file must not cost the headline
                result["config_real_dem"] = {"error": str(exc)[:300], "data": f"real DEM {real_path}"}
    if args.full and rank == 0 and world == 1 and not args.no_configs:
        result["configs"] = other_configs(dem, cam, kw, args, local_rank)
        # roofline rows of these configurations' dominant kernels (and of the multi-GPU strip form) from the rocprofv3 passes
        # committed under profiles/ (tools/gpu_profile_config.sh -> tools/config_rooflines.py): quoted only for THESE kernel sources
        try:
            for path in sorted((ROOT / "profiles").glob("r*_config_rooflines.json"), reverse=True):
                rows = json.loads(path.read_text())
                if any(r.get("kernel_source_hash") != result["kernel_source_hash"] for r in rows.values()):
                    continue
                # (the other configurations' kernels live in other files than the frame kernel's: the whole library's digest)
                from forge3d_amd import _native

                library = _native.source_digest()[:16]
                rows = {k: r for k, r in rows.items() if r.get("library_source_digest") == library or k.startswith("strip") or k == "C4_standin"}
                for key, dest in (("C4_standin", "C4_standin"), ("C3_gi", "C3_gi")):
                    if key in rows and dest in result["configs"] and "error" not in result["configs"][dest]:
                        result["configs"][dest]["profiled_kernel"] = rows[key]
                if "C5" in result["configs"] and "error" not in result["configs"]["C5"]:
                    result["configs"]["C5"]["profiled_kernels"] = {k[3:]: rows[k] for k in ("C5_march", "C5_march_collect", "C5_march_shade", "C5_solver_jacobi") if k in rows}
                result["strip_form_profiled_kernels"] = {k: rows[k] for k in ("strip_trace", "strip_merge", "strip_fused") if k in rows}
                break
        except Exception:  # noqa: BLE001 -- a report, never a reason to lose the line
            pass
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, last_image)
    if rank == 0:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
