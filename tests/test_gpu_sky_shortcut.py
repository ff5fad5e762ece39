"""Certified-sky pixels on the device (csrc/f3d_shade.h sample_primary, csrc/f3d_frame.h frame_lanes): images with a sky
band, a silhouette and edges that are no tile multiples, through the fused kernel with 4 and 8 sample lanes and through the
frames-in-flight pipeline (k_trace / k_merge), over a frame that re-sorts the tiles (k_tile_order).  Every output equals
the oracle's, bit for bit."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import scenes
from test_primary_start import _cliff_dem

pytestmark = pytest.mark.gpu

FRAMES = 6


def _cliff():
    cam = {"origin": (30.0, 22.0, 36.0), "look_at": (0.0, 2.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 40.0, "exposure": 1.0}
    kw = dict(spacing=(1.0, 1.0), exaggeration=1.0, sun_azimuth_deg=200.0, sun_elevation_deg=30.0, earth_model="flat",
              refraction_model="none", seed=11)
    return _cliff_dem(), (64, 48), cam, kw


def _crop():
    dem = scenes.golden_dem(1)[64:192, 64:192].copy()  # 128 x 128
    kw = dict(scenes.scene_kwargs(dem), seed=5)
    cam = {"origin": (20.0, 24.0, 95.0), "look_at": (6.0, 12.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 50.0, "exposure": 1.0}
    return dem, (160, 96), cam, kw


def _cliff_env():
    """The cliff scene under a 4 x 2 environment map of distinct texels: a miss's radiance depends on its direction, so a
    wave of certified sky must keep its sample loop."""
    dem, size, cam, kw = _cliff()
    env = (np.arange(24, dtype=np.float32).reshape(2, 4, 3) * 0.07 + 0.1).astype(np.float32)
    return dem, size, cam, dict(kw, env_map=env)


SCENES = {"cliff 64x48": _cliff, "crop 160x96": _crop, "cliff 64x48, environment map": _cliff_env}


@functools.lru_cache(maxsize=None)
def _want(name):
    """The oracle's render, once per scene, shared by the cases and never modified."""
    from oracle import oracle

    dem, size, cam, kw = SCENES[name]()
    return oracle.render(dem, size[0], size[1], cam, **scenes.fixed_frames(kw, FRAMES, spp=8))


@pytest.mark.parametrize("opts", [dict(kernel_variant=4000000, frames_in_flight=0), dict(kernel_variant=8000000, frames_in_flight=0),
                                  dict(frames_in_flight=4)], ids=["fused S=4", "fused S=8", "in flight"])
@pytest.mark.parametrize("name", list(SCENES))
def test_sky_band_silhouette_and_ragged_edges_are_the_oracles_bits(name, opts):
    from forge3d_amd.session import TerrainSession

    dem, size, cam, kw = SCENES[name]()
    want = _want(name)
    sky = ~np.isfinite(want["depth"])
    assert 0.15 < sky.mean() < 0.85, sky.mean()  # a sky band and terrain, with a silhouette between them
    with TerrainSession(dem, size[0], size[1], cam, **opts, **scenes.fixed_frames(kw, FRAMES, spp=8)) as s:
        s.enqueue_frames(0, FRAMES, True)
        m2, bad = s.window_stats()
        got = s.resolve(FRAMES)
    assert not bad
    assert np.float32(max(0.0, m2) / np.float32(FRAMES - 1)) == np.float32(want["variance"])
    for key in ("rgba", "albedo", "normal", "depth"):
        assert np.array_equal(got[key], want[key], equal_nan=True), (name, opts, key)
