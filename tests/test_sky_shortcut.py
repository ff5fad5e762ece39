"""Certified-sky pixels (csrc/f3d_cone.h kClearForever): a camera sample of such a pixel is a miss without its ray
(f3d_shade.h sample_primary), and a wave whose whole tile is certified, under a uniform environment and without a mesh,
parks the samples' constant sum and skips its sample loop (f3d_frame.h frame_lanes: device code, checked against the
oracle in test_gpu_sky_shortcut.py; the emulator takes every pixel through sample_primary).  Neither may change a bit of
any output, and the certificates for a cone that passes beside the footprint, or leaves it before it comes down, must be
conservative.  F3D_EMUL_NO_SKY_SHORTCUT (f3d_cone.h sky_shortcut_enabled, host builds only) is the shortcut's switch."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import scenes
from emul import emul
from oracle import oracle
from test_primary_start import CAMERAS, _cliff_dem

KW = dict(spacing=(1.0, 1.0), exaggeration=1.0, sun_azimuth_deg=200.0, sun_elevation_deg=30.0, max_frames=3, min_frames=3,
          variance_threshold=1e30, earth_model="flat", refraction_model="none", seed=11)
MIXED = [c for c in CAMERAS if c[0] in ("up at the sky", "above, outside", "along the footprint's edge")]
SIZES = [(35.0, (57, 41)), (110.0, (9, 7))]
ENV_4x2 = (np.arange(24, dtype=np.float32).reshape(2, 4, 3) * 0.07 + 0.1).astype(np.float32)  # 8 distinct texels
SIDE_CAM = {"origin": (6.0, 14.0, 62.0), "look_at": (30.0, 3.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 60.0, "exposure": 1.0}


def _cam(cam, fov):
    return {**cam, "up": (0.0, 1.0, 0.0), "fov_y": fov, "exposure": 1.0}


@functools.lru_cache(maxsize=None)
def _oracle(name, fov, size, spp, env):
    """The oracle's render of a cliff scene (or its error), computed once and shared; never modified."""
    cam = _cam(dict(CAMERAS)[name], fov)
    extra = {"env_map": ENV_4x2} if env else {}
    try:
        return oracle.render(_cliff_dem(), size[0], size[1], cam, dump_state=True, spp=spp, **KW, **extra)
    except RuntimeError as exc:
        return str(exc)


def _emul(dem, size, cam, shortcut=True, **kw):
    if not shortcut:
        os.environ["F3D_EMUL_NO_SKY_SHORTCUT"] = "1"
    try:
        return emul.render(dem, size[0], size[1], cam, **kw)
    finally:
        os.environ.pop("F3D_EMUL_NO_SKY_SHORTCUT", None)


def _same_as_oracle(got, want, tag):
    """Image, AOVs, accumulation and Welford state against the oracle's.  (The temporal reservoirs `res` have no counterpart
    among the oracle's dumps -- it keeps the reservoirs AFTER its spatial pass, which the product evaluates lazily in the
    next frame's head -- so they are compared with the run without the shortcut, whose other state is the oracle's.)"""
    for key in ("rgba", "albedo", "normal", "depth"):
        assert np.array_equal(got[key], want[key], equal_nan=True), (tag, key)
    assert got["frames"] == want["frames"] and np.float32(got["variance"]) == np.float32(want["variance"]), tag
    assert np.array_equal(got["accum"][:, :3], want["accum"][:, :3]), (tag, "accum")
    assert np.array_equal(got["accum"][:, 3], want["welford"][:, 0]), (tag, "welford mean")
    assert np.array_equal(got["m2"], want["welford"][:, 1]), (tag, "m2")


def _certified(dem, size, cam, **geo):
    pixels = [(x, y) for y in range(size[1]) for x in range(size[0])]
    starts = emul.primary_start(dem, size[0], size[1], cam, pixels, **geo)
    return pixels, np.array([s[0] > 1e37 or (int(s[1]) & 0x80000000) != 0 for s in starts])  # (f3d_cone.h: 3e38, or kSkyBeyond)


@pytest.mark.parametrize("spp", [4, 5])
@pytest.mark.parametrize("lanes", [1, 4, 8])
@pytest.mark.parametrize("fov,size", SIZES)
@pytest.mark.parametrize("name,cam", MIXED, ids=[c[0] for c in MIXED])
def test_mixed_tiles_are_the_oracles_bits_with_and_without_the_shortcut(name, cam, fov, size, lanes, spp):
    """Images with all-sky, all-terrain and mixed tiles, 1 / 4 / 8 sample lanes, a ragged last round (spp 5), 3 frames:
    every output and every piece of state equals the oracle's and the emulator's own run with the shortcut off.  A camera
    that sees no terrain ends with the reference's render error on every side."""
    want = _oracle(name, fov, size, spp, False)
    dem, kw = _cliff_dem(), dict(KW, spp=spp, sample_lanes=lanes)
    if isinstance(want, str):
        assert "no valid reservoirs" in want
        for shortcut in (True, False):
            with pytest.raises(RuntimeError, match="no valid reservoirs"):
                _emul(dem, size, _cam(cam, fov), shortcut, **kw)
        return
    on, off = (_emul(dem, size, _cam(cam, fov), shortcut, **kw) for shortcut in (True, False))
    for key in ("rgba", "albedo", "normal", "depth", "accum", "m2", "res"):
        assert np.array_equal(on[key], off[key], equal_nan=True), (name, key)
    _same_as_oracle(on, want, name)


def test_the_mixed_scenes_hold_sky_tiles_terrain_tiles_and_mixed_tiles():
    """What the test above rests on: with 4 sample lanes (4 x 4 tiles) the 57 x 41 images have tiles of all three kinds."""
    kinds = set()
    for name, cam in MIXED[1:]:  # ("up at the sky" is sky only)
        _, sky = _certified(_cliff_dem(), (57, 41), _cam(cam, 35.0), spacing=(1.0, 1.0), exaggeration=1.0)
        sky = sky.reshape(41, 57)
        for ty in range(0, 41, 4):
            for tx in range(0, 57, 4):
                t = sky[ty:ty + 4, tx:tx + 4]
                kinds.add("sky" if t.all() else ("terrain" if not t.any() else "mixed"))
    assert kinds == {"sky", "terrain", "mixed"}, kinds


@pytest.mark.parametrize("lanes", [4, 8])
@pytest.mark.parametrize("fov,size", SIZES)
@pytest.mark.parametrize("name,cam", MIXED, ids=[c[0] for c in MIXED])
def test_an_environment_map_keeps_the_sample_loop(name, cam, fov, size, lanes):
    """With a map of distinct texels a miss's radiance depends on its direction: the per-sample shortcut applies (no ray),
    the per-wave one must not (the samples' sum is no constant)."""
    want = _oracle(name, fov, size, 5, True)
    kw = dict(KW, spp=5, sample_lanes=lanes, env_map=ENV_4x2)
    if isinstance(want, str):
        with pytest.raises(RuntimeError, match="no valid reservoirs"):
            _emul(_cliff_dem(), size, _cam(cam, fov), **kw)
        return
    _same_as_oracle(_emul(_cliff_dem(), size, _cam(cam, fov), **kw), want, name)


# A camera high over the far corner, looking down across the DEM: its upper rows pass over the terrain and leave the
# footprint through the far edges while still descending.
OVER_CAM = {"origin": (44.0, 42.0, 52.0), "look_at": (-6.0, 4.0, -8.0), "up": (0.0, 1.0, 0.0), "fov_y": 55.0, "exposure": 1.0}


@pytest.mark.parametrize("case,cam,kind", [("off to the side", SIDE_CAM, "beside"), ("over and out", OVER_CAM, "leaving")])
def test_sky_certificates_are_conservative_and_reach_new_pixels(case, cam, kind):
    """The centre ray and the four jitter-corner rays of every pixel certified "meets no terrain" miss in the oracle's
    trace.  Among those pixels are ones that held no such certificate before: "beside" -- the centre ray misses the
    footprint altogether (a camera whose image lies partly off the footprint's side); "leaving" -- the centre ray crosses
    the footprint and descends (a cone that comes down only after it has left)."""
    dem, (W, H) = _cliff_dem(), (64, 48)
    pixels, sky = _certified(dem, (W, H), cam, spacing=(1.0, 1.0), exaggeration=1.0)
    origin = np.array(cam["origin"], np.float64)
    fwd = np.array(cam["look_at"], np.float64) - origin
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array(cam["up"], np.float64))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    half_h = np.tan(np.radians(cam["fov_y"]) / 2)
    half_w = half_h * W / H
    plane = np.hypot(half_w / W, half_h / H)
    delta = 1.01 * plane * (1 + plane * plane)
    rays, new = [], {"beside": 0, "leaving": 0}
    half = 0.5 * (dem.shape[0] - 1)
    for (gx, gy), certified in zip(pixels, sky):
        if not certified:
            continue
        for jx, jy in ((0, 0), (-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), (0.5, 0.5)):
            v = np.array([(((gx + 0.5 + jx) / W) * 2 - 1) * half_w, ((1 - (gy + 0.5 + jy) / H) * 2 - 1) * half_h, -1.0])
            v /= np.linalg.norm(v)
            d = v[0] * right + v[1] * up - v[2] * fwd
            d /= np.linalg.norm(d)
            rays.append([*origin, 1e-3, *d, 1e30])
            if (jx, jy) == (0, 0):  # the centre ray against the footprint, grown / shrunk by 0.01: no doubt about its f32 slab test
                def crosses(grow):
                    with np.errstate(divide="ignore", invalid="ignore"):
                        tx = np.sort((np.array([-half - grow, half + grow]) - origin[0]) / d[0])
                        tz = np.sort((np.array([-half - grow, half + grow]) - origin[2]) / d[2])
                    return max(tx[0], tz[0], 1e-3) <= min(tx[1], tz[1])
                new["beside"] += not crosses(0.01)
                new["leaving"] += bool(crosses(-0.01) and d[1] - delta < -1e-3)  # (the old rule asked for d.y - delta >= 0)
    hit = oracle.terrain_trace_batch(dem, np.array(rays, np.float32), origin=(-half, -half), spacing=(1.0, 1.0), exaggeration=1.0,
                                     any_hit=False, apply_curvature=False)
    assert not hit["hit"].any(), [pixels[k // 5] for k in np.flatnonzero(hit["hit"])][:8]
    assert new[kind] >= 1, f"{new} pixels newly certified, {int(sky.sum())} certified in all, of {W * H}"
    assert 0 < int(sky.sum()) < W * H  # (and the image is not all sky)
    # the render itself: the oracle's, with and without the shortcut
    kw = dict(KW, spp=4, sample_lanes=4)
    want = oracle.render(dem, W, H, cam, dump_state=True, **{k: v for k, v in kw.items() if k != "sample_lanes"})
    on, off = (_emul(dem, (W, H), cam, shortcut, **kw) for shortcut in (True, False))
    for key in ("rgba", "albedo", "normal", "depth", "accum", "m2", "res"):
        assert np.array_equal(on[key], off[key], equal_nan=True), key
    _same_as_oracle(on, want, case)


@pytest.mark.parametrize("lanes", [1, 4])
def test_a_mesh_in_front_of_certified_sky_is_seen(lanes):
    """The certificate promises nothing about triangles: with a mesh in the scene both shortcuts are off, and a quad that
    stands in front of certified-sky pixels is in the image."""
    from test_emul_parity import QUAD_I, QUAD_V

    dem = scenes.golden_dem(4)
    kw = scenes.fixed_frames(scenes.scene_kwargs(dem), 3, spp=4, mesh_vertices=QUAD_V, mesh_indices=QUAD_I)
    size = (80, 64)
    want = oracle.render(dem, size[0], size[1], scenes.CAM, dump_state=True, **kw)
    _same_as_oracle(_emul(dem, size, scenes.CAM, sample_lanes=lanes, **kw), want, "mesh")
    _, sky = _certified(dem, size, scenes.CAM, spacing=kw["spacing"], exaggeration=kw["exaggeration"])
    on_mesh = want["albedo"][..., 2].reshape(-1) > 0.7  # (the mesh's albedo: 0.7, 0.7, 0.8)
    assert int((sky & on_mesh).sum()) > 50, int((sky & on_mesh).sum())


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_an_image_of_sky_alone_is_the_references_error(lanes):
    cam = _cam(dict(CAMERAS)["up at the sky"], 35.0)
    kw = dict(KW, spp=4)
    with pytest.raises(RuntimeError, match="no valid reservoirs"):
        oracle.render(_cliff_dem(), 57, 41, cam, **kw)
    with pytest.raises(RuntimeError, match="no valid reservoirs"):
        _emul(_cliff_dem(), (57, 41), cam, sample_lanes=lanes, **kw)
