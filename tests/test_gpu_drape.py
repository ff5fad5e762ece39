"""An image draped over the terrain of a live session (f3d_session_drape; TerrainSession.drape) on the device.

DEMs of 33x33 and 65x63 samples, 96x64 images, spp 1-2, at most 3 frames.

1. tie to the oracle: a constant drape ``c`` (half-representable), under both filters, is bit-identical to a session created with
   ``albedo=c`` -- rgba, albedo, normal, depth, variance and frames -- terrain-only and with a mesh, sample lanes 1 and 4;
2. device equals host body: a random 8x8 and a 40x24 drape give the images of the host frames of
   tests/test_session_drape_host.py (the product's lane bodies with DRAPE = true), both filters;
3. where the texel is taken: under the nearest filter the albedo AOV of every terrain pixel is NumPy's lookup at the point pick()
   reports; mesh pixels read (0.7, 0.7, 0.8), sky pixels 0;
4. per-sample use: a drape black on its left half and ``c`` on its right -- away from the boundary the black side is exactly
   black and the ``c`` side equals the ``albedo=c`` session's frame;
5. life cycle: a patched window equals a fresh session draped with the patched image; drape(None) equals a session never draped;
   a drape survives rearm, reaim, remesh and reterrain; the tensor form equals the host form; NO_WAIT followed by frames;
6. every refusal carries its message and leaves the session's bytes as they were.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_session_drape_host import (CAM, CONSTANT, contract_coords, contract_pack, contract_sample, drape_dem, drape_kw, f32, harness,  # noqa: F401
                                     host_frames, random_image, registration, unpack)

pytestmark = pytest.mark.gpu

W, H = 96, 64
AOVS = ("rgba", "albedo", "normal", "depth")
MESH_ALBEDO = np.array([0.7, 0.7, 0.8], f32).astype(np.float16).astype(f32)


def _session(dem, kw, cam=None, lanes=0, **opts):
    from forge3d_amd.session import TerrainSession, kernel_variant

    return TerrainSession(dem, W, H, dict(cam or CAM), kernel_variant=kernel_variant(sample_lanes=lanes), **opts, **kw)


def _frames(s, n):
    s.enqueue_frames(0, n)
    return s.resolve(n)


def _same(got, want, what, keys=AOVS):
    for key in keys:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key}"


def _constant(shape=(8, 8), c=CONSTANT):
    return np.broadcast_to(np.array(c, f32), (*shape, 3)).copy()


def test_the_library_exports_the_drape():
    from forge3d_amd import _native
    from forge3d_amd.session import TerrainSession

    assert _native.lib().f3d_session_drape is not None and _native.lib().f3d_abi_version() == 6
    assert callable(TerrainSession.drape) and isinstance(TerrainSession.draped, property)


# ---- 1. tie to the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [False, True], ids=["terrain", "mesh"])
@pytest.mark.parametrize("lanes", [1, 4])
def test_a_constant_drape_is_the_session_of_that_albedo(mesh, lanes):
    dem = drape_dem()
    kw = drape_kw(dem, frames=3, spp=2, mesh=mesh)
    with _session(dem, dict(kw, albedo=CONSTANT), lanes=lanes) as s:
        assert s.sample_lanes() == lanes and not s.draped
        want = s.render()
    assert want["frames"] == 3
    assert (want["albedo"] == np.array(CONSTANT, f32)).all(-1).any(), "the camera sees terrain"
    if mesh:
        assert (want["albedo"] == MESH_ALBEDO).all(-1).any(), "the camera sees the mesh"
    for filt in ("nearest", "bilinear"):
        with _session(dem, kw, lanes=lanes) as s:
            s.drape(_constant(), filter=filt)
            assert s.draped and s.drape_info() == {"rows": 8, "cols": 8, "filter": filt, "bytes": 64 + 8 * 8 * 8}
            got = s.render()
        _same(got, want, f"{filt}, {lanes} lanes")
        assert got["frames"] == want["frames"] and got["variance"] == want["variance"] and got["converged"] == want["converged"]


# ---- 2. device equals host body ---------------------------------------------------------------------------------------------------
CASES = [((33, 33), (8, 8), False, 0, "area"), ((63, 65), (24, 40), True, 4, "point")]  # DEM rows x cols, image rows x cols, mesh, lanes


@pytest.fixture(scope="module")
def host_images(harness):  # noqa: F811
    """The host frames of every case and filter (computed once, shared, never written)."""
    out = {}
    for dem_shape, image_shape, mesh, lanes, kind in CASES:
        dem = drape_dem(dem_shape)
        kw = drape_kw(dem, frames=2, spp=2, mesh=mesh)
        image = random_image(image_shape, 41)
        for filt in ("nearest", "bilinear"):
            ref = host_frames(harness, dem, kw, image, filt=filt, kind=kind, lanes=max(lanes, 1), frames=2)
            for v in ref.values():
                v.setflags(write=False)
            out[dem_shape, filt] = ref
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"dem{c[0][1]}x{c[0][0]}-image{c[1][1]}x{c[1][0]}")
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_device_frames_equal_the_host_frames_bit_for_bit(host_images, case, filt):
    dem_shape, image_shape, mesh, lanes, kind = case
    dem = drape_dem(dem_shape)
    kw = drape_kw(dem, frames=2, spp=2, mesh=mesh)
    image = random_image(image_shape, 41)
    want = host_images[dem_shape, filt]
    with _session(dem, kw, lanes=lanes) as s:
        s.drape(image, filter=filt, registration=kind)
        got = _frames(s, 2)
    for key in AOVS:
        wrong = int((got[key] != want[key]).sum()) if key == "rgba" else int((got[key].view(np.uint32) != want[key].view(np.uint32)).sum())
        assert wrong == 0, f"{filt}: {wrong} of {want[key].size} values of {key} differ from the host frames"
    assert len(np.unique(got["albedo"].reshape(-1, 3), axis=0)) > 20, "the image shows"


# ---- 3. where the texel is taken ----------------------------------------------------------------------------------------------------
def test_the_albedo_aov_is_the_texel_under_the_point_pick_reports():
    dem = drape_dem((63, 65))
    kw = drape_kw(dem, frames=1, spp=1, mesh=True)
    image = random_image((8, 8), 43)
    values = unpack(contract_pack(image))
    pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.uint32)
    with _session(dem, kw) as s:
        s.drape(image, filter="nearest")
        hit = s.pick(pixels)
        got = _frames(s, 1)["albedo"].reshape(-1, 3)
    kind = hit["kind"]
    terrain, mesh, sky = kind == 1, kind == 2, kind == 0
    assert terrain.sum() > 1500 and mesh.sum() > 50 and sky.sum() > 50, (int(terrain.sum()), int(mesh.sum()), int(sky.sum()))
    spacing = tuple(f32(v) for v in kw["spacing"])
    origin = (f32(-0.5) * f32(dem.shape[1] - 1) * spacing[0], f32(-0.5) * f32(dem.shape[0] - 1) * spacing[1])
    reg = registration(dem.shape, image.shape, "area")
    p = hit["position"][terrain]
    tx, tz = contract_coords(p[:, 0], p[:, 2], origin, spacing, reg)
    want = contract_sample(values, 0, tx, tz)
    # (a texel boundary under the nearest filter: t + 0.5 on an integer)
    near = (np.abs((tx + 0.5) - np.round(tx + 0.5)) < 1e-3) | (np.abs((tz + 0.5) - np.round(tz + 0.5)) < 1e-3)
    assert near.sum() <= 0.01 * terrain.sum(), f"{int(near.sum())} of {int(terrain.sum())} terrain pixels lie within 1e-3 of a texel boundary"
    wrong = (got[terrain].view(np.uint32) != want.view(np.uint32)).any(1)
    print(f"terrain pixels {int(terrain.sum())}, near a boundary {int(near.sum())}, differing {int(wrong.sum())} (away from boundaries {int((wrong & ~near).sum())})")
    assert not (wrong & ~near).any()
    assert len(np.unique(want, axis=0)) > 20, "the pixels look at many texels"
    assert (got[mesh] == MESH_ALBEDO).all() and (got[sky] == 0.0).all()


# ---- 4. per-sample use ------------------------------------------------------------------------------------------------------------
def _dilate(mask, r):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            shifted = np.zeros_like(mask)
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            shifted[yd, xd] = mask[ys, xs]
            out |= shifted
    return out


def test_every_sample_takes_the_albedo_under_its_own_hit():
    dem = drape_dem()
    kw = drape_kw(dem, frames=1, spp=2)
    c = np.array(CONSTANT, f32)
    image = np.zeros((8, 8, 3), f32)
    image[:, 4:] = c
    with _session(dem, dict(kw, albedo=CONSTANT)) as s:
        want = _frames(s, 1)
    with _session(dem, kw) as s:
        s.drape(image, filter="nearest")
        got = _frames(s, 1)
    terrain = ~np.isnan(got["depth"])
    assert terrain.sum() > 2000 and np.array_equal(np.isnan(got["depth"]), np.isnan(want["depth"]))
    # A boundary pixel: its centre albedo differs from a 3x3 neighbour's -- or its neighbour is sky: black terrain and the sky
    # both read albedo 0, and a jittered sample of a silhouette pixel that escapes to the sky brings the environment, not
    # the drape (the hit kind is told apart by the depth AOV's NaN).
    centre = np.concatenate([got["albedo"], np.isnan(got["depth"])[..., None].astype(f32)], -1)
    boundary = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            boundary[yd, xd] |= (centre[yd, xd] != centre[ys, xs]).any(-1)
    excluded = _dilate(boundary, 2)  # (the jitter of a sample is at most half a pixel)
    assert (excluded & terrain).sum() <= 0.25 * terrain.sum(), f"{int((excluded & terrain).sum())} of {int(terrain.sum())} terrain pixels excluded"
    black = terrain & ~excluded & (got["albedo"] == 0.0).all(-1)
    lit = terrain & ~excluded & (got["albedo"] == c).all(-1)
    print(f"terrain pixels {int(terrain.sum())}, excluded {int((excluded & terrain).sum())}, black {int(black.sum())}, c {int(lit.sum())}, "
          f"black pixels that are not black {int((got['rgba'][black] != np.array([0, 0, 0, 255], np.uint8)).any(-1).sum())}")
    assert black.sum() > 300 and lit.sum() > 300 and (black | lit | excluded | ~terrain).all(), (int(black.sum()), int(lit.sum()))
    assert (got["rgba"][black] == np.array([0, 0, 0, 255], np.uint8)).all(), "a sample on the black half reflects nothing"
    assert np.array_equal(got["rgba"][lit], want["rgba"][lit]), "the samples on the other half reflect c"
    assert (want["rgba"][black][:, :3] != 0).any(), "(the albedo=c session is not black there)"
    # the boundary itself mixes the two: some pixel there is neither
    mixed = boundary & terrain & (got["rgba"][..., :3] != 0).any(-1) & (got["rgba"] != want["rgba"]).any(-1)
    assert mixed.any(), "a pixel on the boundary holds samples of both halves"


# ---- 5. life cycle ------------------------------------------------------------------------------------------------------------------
ORBIT = {"origin": (63.6, 45.0, 63.6), "look_at": (0.0, 5.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}


def test_a_patched_window_equals_a_fresh_session_draped_with_the_patched_image():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    image, window = random_image((24, 40), 51), random_image((5, 7), 52, channels=4)
    patched = image.copy()
    patched[9:14, 30:37] = window[..., :3]
    with _session(dem, kw) as fresh:
        fresh.drape(patched, registration="point")
        want = _frames(fresh, 2)
        bytes_want = fresh.info()["gpu_resource_bytes"]
    with _session(dem, kw) as s:
        s.drape(image, registration="point")
        first = _frames(s, 2)
        before = s.info()["gpu_resource_bytes"]
        s.drape(window, at=(9, 30))
        assert s.drape_info()["rows"] == 24 and s.drape_info()["filter"] == "bilinear"
        got = _frames(s, 2)
        assert s.info()["gpu_resource_bytes"] == before, "a window takes nothing (its rows fit the slab of the whole image)"
        assert before == bytes_want
    assert not np.array_equal(first["rgba"], got["rgba"])
    _same(got, want, "patched")


def test_removing_the_drape_leaves_a_session_that_was_never_draped():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2, mesh=True)
    with _session(dem, kw) as never:
        want = never.render()
        bytes_never = never.info()["gpu_resource_bytes"]
        fp_never = never.fingerprint()
    with _session(dem, kw) as s:
        s.drape(random_image((8, 8), 53))
        draped = s.render()
        assert s.info()["gpu_resource_bytes"] > bytes_never
        s.drape(None)
        assert not s.draped and s.drape_info() is None
        got = s.render()
        assert s.info()["gpu_resource_bytes"] == bytes_never
        assert {k: v for k, v in s.fingerprint().items() if k != "frame_heads"} == {k: v for k, v in fp_never.items() if k != "frame_heads"}
        s.drape(None)  # (nothing to remove: a re-aim)
        _same(s.render(), want, "removed twice")
    assert not np.array_equal(draped["rgba"], want["rgba"])
    _same(got, want, "removed")
    assert got["frames"] == want["frames"] and got["variance"] == want["variance"]


def test_a_drape_survives_the_other_updates():
    dem = drape_dem()
    verts, tris = scenes.box_city(n_boxes=12, seed=5, span=0.9 * scenes.SPAN, top=14.0)
    kw = drape_kw(dem, frames=2, spp=2, mesh=True)
    image = random_image((8, 8), 54)
    moved = (verts + np.array([3.0, 1.0, -2.0], f32)).astype(f32)
    dem2 = (dem * f32(0.8) + f32(0.1)).astype(f32)
    steps = [("rearm", lambda s: s.rearm(sun_azimuth_deg=80.0, seed=11), dict(kw, sun_azimuth_deg=80.0, seed=11), dem, CAM),
             ("reaim", lambda s: s.reaim(ORBIT), dict(kw, sun_azimuth_deg=80.0, seed=11), dem, ORBIT),
             ("remesh", lambda s: s.remesh(moved), dict(kw, sun_azimuth_deg=80.0, seed=11, mesh_vertices=moved), dem, ORBIT),
             ("reterrain", lambda s: s.reterrain(dem2), dict(kw, sun_azimuth_deg=80.0, seed=11, mesh_vertices=moved), dem2, ORBIT)]
    with _session(dem, kw) as s:
        s.drape(image, filter="nearest")
        for name, update, fresh_kw, fresh_dem, cam in steps:
            update(s)
            assert s.draped, name
            got = _frames(s, 2)
            with _session(fresh_dem, fresh_kw, cam=cam) as fresh:
                fresh.drape(image, filter="nearest")
                want = _frames(fresh, 2)
            _same(got, want, f"after {name}")
            assert len(np.unique(got["albedo"].reshape(-1, 3), axis=0)) > 10, name


def test_the_tensor_form_equals_the_host_form_and_no_wait_is_ordered():
    import torch

    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    image, other = random_image((24, 40), 55, channels=4), random_image((24, 40), 56)
    with _session(dem, kw) as s:
        s.drape(image)
        want = _frames(s, 2)
        s.drape(other)
        want_other = _frames(s, 2)
        slab = s.info()["gpu_resource_bytes"]
    with _session(dem, kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        d_image = torch.from_numpy(image).cuda()
        s.drape(d_image)
        assert s.info()["gpu_resource_bytes"] == bytes0 + 64 + 24 * 40 * 8, "the device form takes the drape and no slab"
        assert slab == bytes0 + 64 + 24 * 40 * 8 + 24 * 40 * 4 * 4, "the host form: the drape and the slab of its widest image"
        _same(_frames(s, 2), want, "tensor form")
        d_other = torch.from_numpy(other).cuda()
        s.drape(d_other, wait=False)  # NO_WAIT: the packing kernel is in flight on the session's stream (the null stream here)
        s.enqueue_frames(0, 2)
        got = s.resolve(2)
        _same(got, want_other, "tensor form, no wait, frames right behind it")
        # what a half cannot hold is stored as 0 in the device form (nobody can look)
        bad = torch.from_numpy(other).cuda()
        bad[3, 5, 1] = float("nan")
        bad[4, 6, 0] = -1.0
        bad[5, 7, 2] = 1e6
        s.drape(bad, filter="nearest", registration="point")
        zeroed = other.copy()
        zeroed[3, 5, 1] = zeroed[4, 6, 0] = zeroed[5, 7, 2] = 0.0
        got_bad = _frames(s, 2)
        s.drape(zeroed, filter="nearest", registration="point")
        _same(_frames(s, 2), got_bad, "non-finite, negative and too large texels of a tensor are zeros")
        with pytest.raises(ValueError, match="a tensor drape needs a tensor on the session's device"):
            s.drape(torch.from_numpy(image))
        with pytest.raises(ValueError, match="a tensor drape must be float32"):
            s.drape(d_image.double())
        with pytest.raises(ValueError, match="wait=False needs a contiguous tensor"):
            s.drape(d_image[:, ::2], wait=False)
        s.drape(d_image[:, ::2])  # (waited for: the copy lives as long as the call)


def test_load_overlay_renders_what_a_draped_session_renders(tmp_path):
    from forge3d_amd import io as f3d_io
    from forge3d_amd.session import TerrainSession
    from forge3d_amd.viewer import ViewerHandle

    dem = drape_dem()
    image = (random_image((24, 40), 57) * 255).astype(np.uint8)
    extent = (0.25, 0.0, 0.75, 0.5)
    f3d_io.numpy_to_png(tmp_path / "ortho.png", image)
    v = ViewerHandle(W, H, spp=2, max_frames=2, min_frames=2, variance_threshold=1e30)
    v.load_terrain(dem, scenes.SPAN / (dem.shape[1] - 1))
    v.set_z_scale(scenes.RELIEF)
    keys = [dict(phi_deg=28.0, theta_deg=49.0, radius=120.0, fov_deg=60.0), dict(phi_deg=70.0, theta_deg=55.0, radius=110.0, fov_deg=40.0)]
    v.set_orbit_camera(**keys[0])
    plain = v.render()
    v.load_overlay("ortho", tmp_path / "ortho.png", extent=extent, filter="nearest")
    got = v.render()
    assert not np.array_equal(got["rgba"], plain["rgba"])
    wanted = []
    for key in keys:
        v.set_orbit_camera(key["phi_deg"], key["theta_deg"], key["radius"], key.get("fov_deg"))
        d, w, h, camera, keywords = v._call()
        with TerrainSession(d, w, h, camera, **keywords) as s:
            s.drape(image, filter="nearest", srgb=True, registration=ViewerHandle.overlay_registration(dem.shape, image.shape, extent))
            wanted.append(s.render())
    _same(got, wanted[0], "load_overlay + render")
    assert got["frames"] == wanted[0]["frames"] == 2 and len(np.unique(got["albedo"].reshape(-1, 3), axis=0)) > 20
    # an animation: one draped session re-aimed per key writes what a fresh draped session per key renders
    v.render_animation(keys, tmp_path / "frames")
    for i, want in enumerate(wanted):
        assert np.array_equal(f3d_io.png_to_numpy(tmp_path / "frames" / f"frame_{i:04d}.png"), want["rgba"]), f"key {i}"
    v.remove_overlay("ortho")
    v.set_orbit_camera(**keys[0])
    _same(v.render(), plain, "overlay removed")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def _raw(s, image=None, **members):
    """f3d_session_drape with a descriptor of the caller's: (status, message)."""
    from forge3d_amd import _native

    q = _native.DrapeDesc()
    q.struct_size = C.sizeof(_native.DrapeDesc)
    if image is not None:
        q.image = image.ctypes.data
        q.rows, q.cols, q.channels = image.shape
    q.filter = _native.DRAPE_BILINEAR
    q.scale_x, q.offset_x, q.scale_z, q.offset_z = 0.25, -0.5, 0.25, -0.5
    q.aim = s._aim(None, {})
    for k, v in members.items():
        setattr(q, k, v)
    err = C.create_string_buffer(1024)
    rc = s._lib.f3d_session_drape(s._handle, C.byref(q), err, len(err))
    return rc, err.value.decode()


def _state(s):
    return s.fingerprint(), s.info()["gpu_resource_bytes"], s.drape_info()


def test_every_refusal_leaves_the_session_as_it_was():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    good = random_image((8, 8), 61)
    with _session(dem, kw) as s:
        s.enqueue_frames(0, 1)
        undraped = _state(s)

        def refused(status, match, image=good, state=undraped, **members):
            rc, message = _raw(s, image, **members)
            assert rc == status and match in message, (rc, message)
            assert _state(s) == state, f"after the refusal '{match}'"

        for bad, what in ((np.nan, "non-finite"), (np.inf, "non-finite"), (-1e-3, "negative"), (65505.0, "too large")):
            image = good.copy()
            image[7, 7, 2] = bad
            refused(3, "drape texels must be finite and >= 0", image)
            with pytest.raises(RuntimeError, match="drape texels must be finite and >= 0"):
                s.drape(image)
        rgba = random_image((8, 8), 62, channels=4)
        rgba[2, 2, 3] = np.nan  # (the fourth channel is not read)
        assert _raw(s, rgba)[0] == 0 and s.draped
        s.drape(None)
        assert _state(s)[1:] == undraped[1:]
        undraped = _state(s)
        refused(1, "a drape has 3 or 4 channels", state=undraped, channels=5)
        refused(1, "a drape has 3 or 4 channels", state=undraped, channels=1)
        refused(1, "a drape holds 1..16384 texels a side", state=undraped, rows=0)
        refused(1, "a drape holds 1..16384 texels a side", state=undraped, cols=16385)
        refused(1, "registration scales must not be zero", state=undraped, scale_x=0.0)
        refused(1, "registration scales must not be zero", state=undraped, scale_z=-0.0)
        refused(1, "must be finite", state=undraped, offset_z=float("inf"))
        refused(1, "must be finite", state=undraped, scale_x=float("nan"))
        refused(1, "drape filter must be 0 (nearest) or 1 (bilinear)", state=undraped, filter=2)
        refused(1, "unknown drape flags", state=undraped, flags=32)
        refused(1, "NO_WAIT needs DEVICE_POINTERS", state=undraped, flags=8)
        refused(1, "f3d_session_drape_desc", state=undraped, struct_size=8)
        refused(1, "this session has no drape: a window (PATCH)", state=undraped, flags=16)
        refused(1, "they need the PATCH flag", state=undraped, at_row=1)
        refused(1, "a null image removes the drape: it takes no window", None, state=undraped, flags=16)
        with pytest.raises(ValueError, match="this session has no drape"):
            s.drape(good[:2, :2], at=(0, 0))
        with pytest.raises(RuntimeError, match="camera"):  # (the create's own check, through the update's path)
            s.drape(good, {"origin": (0.0, 1.0, 0.0), "look_at": (0.0, 1.0, 0.0)})
        assert _state(s) == undraped
        # with a drape in place: what is refused leaves THAT drape
        s.drape(good, filter="nearest")
        want = _frames(s, 2)
        s.rearm()  # (the render starts again at frame 0)
        s.enqueue_frames(0, 1)
        draped = _state(s)
        for at in ((7, 0), (0, 7), (8, 0), (0, 8)):
            refused(1, "leaves the session's 8x8 drape", good[:2, :2].copy(), state=draped, flags=16, at_row=at[0], at_col=at[1])
        image = good.copy()
        image[0, 0, 0] = np.nan
        refused(3, "drape texels must be finite", image, state=draped)
        refused(3, "drape texels must be finite", image[:2, :2].copy(), state=draped, flags=16)
        # the frame paths without a draped form name the fused path
        for call, match in ((lambda: s.enqueue_trace(0, 1), "a trace batch (k_trace) has no draped form: a draped session renders through the fused frame path"),
                            (lambda: s.enqueue_merge(0), "a merge of traced frames (k_merge) has no draped form"),
                            (lambda: s.enqueue_frame_part(1, 1), "a frame in two parts (f3d_session_enqueue_frame_part) has no draped form"),
                            (lambda: s.enqueue_batch_strip(1, 1), "a strip batch with peer halos (f3d_session_enqueue_batch_strip) has no draped form")):
            with pytest.raises(ValueError) as e:
                call()
            assert match in str(e.value) and "f3d_session_enqueue_frames" in str(e.value)
            assert _state(s) == draped, match
        s.rearm()
        _same(_frames(s, 2), want, "after the refusals")


def test_sessions_without_a_draped_form_refuse_a_drape():
    from forge3d_amd.session import TerrainSession

    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    good = random_image((8, 8), 63)
    for opts, match in ((dict(frames_in_flight=2), "frames in flight (k_trace / k_merge), which have no draped form: a drape needs the fused frame path"),
                        (dict(kernel_variant=104), "kernel_variant 104 selects a register-budget A/B instantiation"),
                        (dict(kernel_variant=4000105), "kernel_variant 105 selects a register-budget A/B instantiation")):
        with TerrainSession(dem, W, H, dict(CAM), **opts, **dict(kw, spp=4 if opts.get("kernel_variant") == 4000105 else 2)) as s:
            s.enqueue_frames(0, 1)
            before = _state(s)
            with pytest.raises(ValueError) as e:
                s.drape(good)
            assert match in str(e.value), str(e.value)
            assert _state(s) == before and not s.draped
            s.drape(None)  # (nothing to remove: a re-aim, allowed everywhere)
    # connected peer halos: in the words of the other updates
    sessions = [TerrainSession(dem, W, H, dict(CAM), row_begin=b, row_end=e, **kw) for b, e in ((0, 29), (29, 64))]
    try:
        exports = [s.halo_export() for s in sessions]
        sessions[0].halo_connect(1, exports[1])
        sessions[1].halo_connect(0, exports[0])
        for s in sessions:
            before = _state(s)
            with pytest.raises(ValueError, match="a session with peer halos cannot be draped: the frame counters its neighbours poll only rise"):
                s.drape(good)
            assert _state(s) == before
    finally:
        for s in sessions:
            s.close()


def test_a_drape_past_the_memory_budget_is_refused_and_the_old_one_stays():
    dem = drape_dem()
    kw = drape_kw(dem, frames=2, spp=2)
    small, large = random_image((8, 8), 64), random_image((96, 64), 65)
    with _session(dem, kw) as s:
        s.drape(small)
        need = s.info()["gpu_resource_bytes"]
    with _session(dem, kw, memory_budget_bytes=need + 4096) as s:
        s.drape(small)
        want = _frames(s, 2)
        s.rearm()  # (the render starts again at frame 0)
        s.enqueue_frames(0, 1)
        before = _state(s)
        with pytest.raises(RuntimeError, match="drape exceeds the memory budget"):
            s.drape(large)
        assert _state(s) == before
        s.rearm()
        _same(_frames(s, 2), want, "the old drape renders on")
