"""Deep-sky blocks on the device (csrc/f3d_skyblocks.h; csrc/f3d_frame.h k_sky_blocks, k_head, frame_wave): 8 x 8 blocks so
far inside certified sky that k_head settles their pixels (accumulation and Welford state only) and the frame kernel does
nothing for their tiles.  Images with deep blocks, a rim of certified pixels outside them, a silhouette, terrain and edges
that are no multiples of 8, through the fused kernel with 4 and 8 sample lanes, window statistics collected on the last
frame: every output equals the oracle's, bit for bit.  Sessions that cannot use the table (an environment map, frames in
flight) say so and still match.  State that outlives a call: after a re-aim onto terrain and back, a re-arm, a re-terrain
that raises a ridge into the sky and a drape set and removed, the render is a fresh session's; and under an allocator that
fills every buffer with 0xFF both reservoir buffers of the deep pixels stay all-zero."""
from __future__ import annotations

import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import scenes
from test_gpu_sky_shortcut import _cliff, _cliff_env, _crop

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FRAMES = 6
AOVS = ("rgba", "albedo", "normal", "depth")
FUSED = {"fused S=4": dict(kernel_variant=4000000, frames_in_flight=0), "fused S=8": dict(kernel_variant=8000000, frames_in_flight=0)}


def _cliff_up():
    """The cliff scene of test_gpu_sky_shortcut.py with the camera tilted up until the sky is more than a block's rectangle
    deep (checked with the CPU certificate code: 18 of 48 blocks deep -- two block rows and both ends of a third --, 983
    certified pixels around them, 937 pixels of terrain and silhouette)."""
    dem, size, cam, kw = _cliff()
    return dem, size, dict(cam, look_at=(0.0, 16.0, 0.0)), kw


def _cliff_ragged():
    """The same at a size whose width and height are no multiples of 8 (nor of a frame tile), tilted less: 13 of 70 blocks
    deep, among them the ragged ones of the right rim, one block row and the ends of a second."""
    dem, _, cam, kw = _cliff()
    return dem, (75, 53), dict(cam, look_at=(0.0, 8.0, 0.0)), kw


def _cliff_up_env():
    """Under a 4 x 2 environment map of distinct texels a miss's radiance depends on its direction: no block may be settled."""
    dem, size, cam, kw = _cliff_up()
    return dem, size, cam, dict(kw, env_map=_cliff_env()[3]["env_map"])


SCENES = {"cliff 64x48": _cliff_up, "crop 160x96": _crop, "cliff 75x53": _cliff_ragged}


def _kw(kw):
    return scenes.fixed_frames(kw, FRAMES, spp=8)


@functools.lru_cache(maxsize=None)
def _want(name):
    """The oracle's render, once per scene, shared by the cases and never modified."""
    from oracle import oracle

    dem, size, cam, kw = {**SCENES, "cliff 64x48, environment map": _cliff_up_env}[name]()
    return oracle.render(dem, size[0], size[1], cam, **_kw(kw))


def _frames(s):
    """FRAMES frames with the window statistics collected on the last one, and the resolve."""
    s.enqueue_frames(0, FRAMES, True)
    m2, bad = s.window_stats()
    return s.resolve(FRAMES), m2, bad


def _same_as_oracle(got, m2, bad, want, what):
    assert not bad
    assert np.float32(max(0.0, m2) / np.float32(FRAMES - 1)) == np.float32(want["variance"]), what
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


@pytest.mark.parametrize("opts", list(FUSED.values()), ids=list(FUSED))
@pytest.mark.parametrize("name", list(SCENES))
def test_deep_blocks_a_rim_and_terrain_are_the_oracles_bits(name, opts):
    from forge3d_amd.session import TerrainSession

    dem, size, cam, kw = SCENES[name]()
    want = _want(name)
    with TerrainSession(dem, size[0], size[1], cam, **opts, **_kw(kw)) as s:
        sky = s.sky_blocks()
        got, m2, bad = _frames(s)
        assert s.sky_blocks() == sky, "frames leave the table alone"
    # not vacuous: blocks that are settled, certified pixels that are not (the rim: the sky tile and the sample loop), terrain
    assert sky["blocks"] == ((size[0] + 7) // 8) * ((size[1] + 7) // 8)
    assert sky["deep_blocks"] >= 2, sky
    assert sky["certified_pixels"] > sky["deep_pixels"] >= 1, sky
    assert np.isfinite(want["depth"]).sum() >= 64, "terrain"
    assert sky["certified_pixels"] <= (~np.isfinite(want["depth"])).sum(), "a certified pixel is a sky pixel"
    _same_as_oracle(got, m2, bad, want, (name, opts))


@pytest.mark.parametrize("case", ["environment map", "frames in flight"])
def test_sessions_that_cannot_use_the_table_have_no_deep_block_and_still_match(case):
    from forge3d_amd.session import TerrainSession

    name, opts = {"environment map": ("cliff 64x48, environment map", FUSED["fused S=4"]),
                  "frames in flight": ("cliff 64x48", dict(frames_in_flight=4))}[case]
    dem, size, cam, kw = (_cliff_up_env if "environment" in name else _cliff_up)()
    with TerrainSession(dem, size[0], size[1], cam, **opts, **_kw(kw)) as s:
        sky = s.sky_blocks()
        got, m2, bad = _frames(s)
    assert sky["deep_blocks"] == 0 and sky["deep_pixels"] == 0, sky
    _same_as_oracle(got, m2, bad, _want(name), case)


# ---- state that outlives a call ------------------------------------------------------------------------------------------
DOWN = {"origin": (2.0, 40.0, 3.0), "look_at": (0.0, 0.0, 0.0), "up": (0.0, 0.0, -1.0), "fov_y": 40.0, "exposure": 1.0}  # terrain in every pixel


def _ridge(dem):
    """The cliff DEM with a ridge raised behind the wall, into what the cliff camera sees as sky."""
    out = dem.copy()
    out[:, :6] += 40.0
    out[:6, :] += 40.0
    return out


def _render(s):
    got = s.render()
    return {key: got[key] for key in (*AOVS, "frames", "variance")}


def _fresh(dem, size, cam, kw, opts, drape=None):
    from forge3d_amd.session import TerrainSession

    with TerrainSession(dem, size[0], size[1], cam, **opts, **kw) as s:
        if drape is not None:
            s.drape(drape, cam)
        return _render(s), s.sky_blocks()


def _same(got, want, what):
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)
    assert got["frames"] == want["frames"] and got["variance"] == want["variance"], what


@pytest.mark.parametrize("opts", list(FUSED.values()), ids=list(FUSED))
def test_updates_leave_what_a_fresh_session_renders(opts):
    """One session through a chain of updates, each step against a fresh session of that state: the table follows the
    certificates (re-aim, re-terrain), a re-arm leaves it alone, and neither the head records nor the reservoirs of blocks
    that were deep a step ago carry anything into the next render."""
    from forge3d_amd.session import TerrainSession

    dem, size, cam, kw = _cliff_up()
    kw = _kw(kw)
    ridge = _ridge(dem)
    image = (np.linspace(0.1, 0.9, dem.shape[0] * dem.shape[1] * 3, dtype=np.float32).reshape(*dem.shape, 3) ** 2).astype(np.float32)
    rearmed = dict(kw, sun_azimuth_deg=95.0, sun_elevation_deg=12.0, seed=23)
    with TerrainSession(dem, size[0], size[1], cam, **opts, **kw) as s:
        deep0 = s.sky_blocks()
        assert deep0["deep_blocks"] >= 2
        want, sky = _fresh(dem, size, cam, kw, opts)
        _same(_render(s), want, "the create")
        assert sky == deep0

        s.reaim(DOWN)  # the former sky is terrain
        want, sky = _fresh(dem, size, DOWN, kw, opts)
        assert s.sky_blocks() == sky and sky["deep_blocks"] == 0 and sky["certified_pixels"] == 0, sky
        _same(_render(s), want, "re-aimed onto terrain")

        s.reaim(cam)  # and back
        assert s.sky_blocks() == deep0
        _same(_render(s), _fresh(dem, size, cam, kw, opts)[0], "re-aimed back")

        s.rearm(sun_azimuth_deg=95.0, sun_elevation_deg=12.0, seed=23)
        assert s.sky_blocks() == deep0, "a re-arm leaves the table alone"
        _same(_render(s), _fresh(dem, size, cam, rearmed, opts)[0], "re-armed")

        s.reterrain(ridge, cam)  # a ridge into former sky
        want, sky = _fresh(ridge, size, cam, rearmed, opts)
        assert s.sky_blocks() == sky and sky["deep_pixels"] < deep0["deep_pixels"], (sky, deep0)
        _same(_render(s), want, "re-terrained")

        s.reterrain(dem, cam)
        assert s.sky_blocks() == deep0
        s.drape(image, cam)
        assert s.sky_blocks() == deep0, "a draped session keeps its table: the drape is read at hits only"
        _same(_render(s), _fresh(dem, size, cam, rearmed, opts, drape=image)[0], "draped")
        s.drape(None, cam)
        assert s.sky_blocks() == deep0
        _same(_render(s), _fresh(dem, size, cam, rearmed, opts)[0], "the drape removed")


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import torch
import test_gpu_sky_blocks as t
from forge3d_amd.distributed import HipBackend, HALO_ROWS, RES_BYTES
dem, size, cam, kw = t._cliff_up()
w, h = size
backend = HipBackend(0)
nbytes = (h + 2 * HALO_ROWS) * w * RES_BYTES
res = [backend.empty_bytes(nbytes), backend.empty_bytes(nbytes)]
for r in res:
    r.fill_(255)  # (caller-owned buffers are not the allocator's: the pattern by hand)
stats = backend.empty_i32(4)
s = backend.make_session(dem, w, h, cam, 0, h, res, stats, dict(t._kw(kw), **t.FUSED["fused S=4"]))
try:
    sky = s.sky_blocks()
    s.enqueue_frames(0, t.FRAMES, True)
    s.window_stats()
    got = s.resolve(t.FRAMES)
    backend.sync()
    out = {"res%d" % i: r.cpu().numpy().view(np.uint8).reshape(h + 2 * HALO_ROWS, w, RES_BYTES)[HALO_ROWS:HALO_ROWS + h] for i, r in enumerate(res)}
    np.savez(sys.argv[2], rgba=got["rgba"], deep_blocks=sky["deep_blocks"], deep_pixels=sky["deep_pixels"], **out)
finally:
    s.close()
"""


def test_reservoirs_of_deep_pixels_stay_zero_under_a_poisoning_allocator():
    """F3D_POISON=255 in a child process, the reservoir buffers the caller's and pre-filled with 0xFF: after 6 frames both
    buffers hold all-zero records at every pixel of a deep block -- the session's clear, which nothing may overwrite there --
    and the image is the oracle's.  Which pixels are deep: the CPU certificate code and the erosion, checked against the
    diagnostic's counts."""
    from emul import emul

    dem, size, cam, kw = _cliff_up()
    w, h = size
    env = dict(os.environ, F3D_POISON="255")
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "out.npz"
        proc = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-3000:]
        got = dict(np.load(path))
    starts = emul.primary_start(dem, w, h, cam, [(x, y) for y in range(h) for x in range(w)], **kw)
    certified = np.array([np.float32(t) == np.float32(3.0e38) or (level & 0x80000000) != 0 for t, level in starts]).reshape(h, w)
    padded = np.ones((h + 8 + 8, w + 8 + 8), bool)
    padded[4:4 + h, 4:4 + w] = certified
    deep = np.lib.stride_tricks.sliding_window_view(padded, (16, 16))[::8, ::8][:(h + 7) // 8, :(w + 7) // 8].all(axis=(2, 3))
    pixels = np.kron(deep, np.ones((8, 8), bool))[:h, :w]
    assert int(deep.sum()) == int(got["deep_blocks"]) >= 2 and int(pixels.sum()) == int(got["deep_pixels"])
    for i in (0, 1):
        assert not got[f"res{i}"][pixels].any(), f"reservoir buffer {i}: a deep pixel's record is not all-zero"
        assert got[f"res{i}"][~pixels].any(), "the other pixels' reservoirs hold samples"
    assert np.array_equal(got["rgba"], _want("cliff 64x48")["rgba"])
