"""Scenes shared by tests/test_leaf_shortcut.py (emulator) and tests/test_gpu_leaf_shortcut.py (device): data only, no
emulator and no device import."""
from __future__ import annotations

import numpy as np

import scenes


def checkerboard(n=64, relief=1.0):
    z, x = np.mgrid[0:n, 0:n]
    return (((x + z) & 1) * relief).astype(np.float32)  # every patch a saddle: maximal twist


def checker_scene():
    """The checkerboard at exaggeration 37 under a sun 5 degrees up: grazing sun rays over twisted patches."""
    cam = {"origin": (10.0, 75.0, 95.0), "look_at": (0.0, 12.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}
    kw = dict(spacing=(1.0, 1.0), exaggeration=37.0, sun_azimuth_deg=215.0, sun_elevation_deg=5.0, earth_model="flat",
              refraction_model="none", seed=9)
    return checkerboard(), cam, kw


def far_scene():
    """Kilometre spacing on the ellipsoid: the sun rays carry the curvature policy; a low sun, so that many are occluded."""
    dem = scenes.golden_dem(4)
    span = 1000.0 * (dem.shape[1] - 1)
    cam = {"origin": (0.0, 0.35 * span, 0.9 * span), "look_at": (0.0, 0.05 * span, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}
    kw = dict(spacing=(1000.0, 1000.0), exaggeration=0.2 * span, sun_azimuth_deg=225.0, sun_elevation_deg=12.0,
              earth_model="ellipsoid", seed=7)
    return dem, cam, kw
