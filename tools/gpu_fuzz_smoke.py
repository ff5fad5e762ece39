#!/usr/bin/env python
"""Parity fuzz of the smoke ray-marcher on the GPU: N seeded random volumes, cameras, suns and settings through
f3d_smoke_render (perspective and projection) vs oracle/smoke_oracle.c, every byte.  Aimed at what round 5 put around the
reference's loop: the clipping against the smoke's bounding box (smoke at the grid's ends, cameras inside the volume,
axis-parallel rays, voxels much smaller than their distance from the origin), the three-instruction quotients (awkward voxel
sizes), and the chunked list of the deferred self-shadow marches (long rays, a list that runs out).

    python tools/gpu_fuzz_smoke.py [first seed] [count]"""
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from forge3d_amd import smoke  # noqa: E402
from oracle import smoke_oracle  # noqa: E402  (checker only: this is a test tool)
from smoke_march_cases import case  # noqa: E402  (the scenes, shared with the fuzz slice of tests/test_smoke.py)

first, count = (int(sys.argv[1]) if len(sys.argv) > 1 else 1), (int(sys.argv[2]) if len(sys.argv) > 2 else 200)
bad, t0, smoky = [], time.time(), 0
for seed in range(first, first + count):
    fields, vs, og, pos, target, up, fov, sun, view, st, w, h, frame = case(seed)
    if seed % 5 == 0:
        os.environ["F3D_SMOKE_SHADOW_SLOTS"] = "2048"  # a list with room for two chunks
    else:
        os.environ.pop("F3D_SMOKE_SHADOW_SLOTS", None)
    d = fields["density"]
    dom = smoke.SmokeDomain((d.shape[2], d.shape[1], d.shape[0]), vs, og)
    dom.set_density(d)
    dom.set_temperature(fields["temperature"]), dom.set_soot(fields["soot"]), dom.set_humidity(fields["humidity"])
    dom.set_emission(fields["emission_rate"]), dom.set_particle_age(fields["particle_age"])
    dom.frame_index = frame
    settings = smoke.SmokeRenderSettings(**st)
    got = dom.render_rgba(w, h, pos, target, up=up, fovy_deg=fov, sun_direction=sun, settings=settings)
    want = smoke_oracle.render_rgba(fields, w, h, pos, target, up=up, fovy_deg=fov, sun_direction=sun, voxel_size=vs, origin=og, frame_index=frame, **st)
    got_p = dom.render_projection_rgba(w, h, view, sun, settings=settings)
    want_p = smoke_oracle.render_projection_rgba(fields, w, h, view, sun, voxel_size=vs, origin=og, frame_index=frame, **st)
    smoky += int(want[..., 3].any()) + int(want_p[..., 3].any())
    if not np.array_equal(got, want):
        bad.append((seed, "perspective", int((got != want).any(-1).sum())))
    if not np.array_equal(got_p, want_p):
        bad.append((seed, "projection", int((got_p != want_p).any(-1).sum())))
print(f"{count} smoke scenes x 2 views from seed {first}: {len(bad)} mismatches {bad[:10]}, {smoky} of {2 * count} images show smoke, {time.time() - t0:.1f} s")
