"""`-m gpu`: the device against the float64 geometric reference (tests/trace_reference.py), through the product's entry points only.

The sets, the conditions and the gates are those of tests/test_trace_reference_host.py (proof rays, seeded generic ray lists and
whole rasters over the small shapes; 0 disagreements outside the band; height and angle tolerances four times what the oracle
shows, imported from trace_reference.py):

* TerrainSession.trace, occluded(curved=False / True) and ground on the proof set and the small shapes; ground within
  8 ulp(top) of the f64 bilinear patch;
* visibility in the host form and the device-tensor form, viewshed, shadow_mask and sun_hours on every small shape, curved off
  and on; sun_hours equals the sum of the masks; a strip session answers the whole DEM the same way;
* after reterrain of a 16x16 patch of the 64x64 golden DEM, with no host wait: the rasters and a ray list over the NEW heights;
* the box city, mesh builders 0, 2, 3: occluded and visibility against the terrain reference OR the f64 triangle search,
  terrain_only against the terrain reference alone;
* the curved-earth golden scene: the device's curved viewshed equals the f64 reference's bit for bit outside the band; the
  reference's own IoU against the stored golden is printed, the 0.98 gate stays.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import scenes
from test_gpu_reaim import H, W
from test_session_raster_host import (TOWARD, contract_origins, contract_rays, iou, sun_direction, viewshed_targets, whitebox_observer,
                                      whitebox_reference, whitebox_scene_kwargs)
from test_session_raster_host import HostScene as RasterScene
from test_trace_reference_host import (LIFTS, PROOF_CAM, RASTER_SHAPES, SHAPES, SUNS, CitySets, TraceSet, city_raster_targets, city_scene,
                                       describe, gate_city, gate_closest, gate_occlusion, list_rays, proof_scene, raster_bits, raster_lib, raster_rays,
                                       reterrain_case, shape_scene)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _session(dem, kw, cam=None, **opts):
    from forge3d_amd.session import TerrainSession

    return TerrainSession(dem, W, H, dict(cam or scenes.CAM), **opts, **kw)


def _constants(dem, kw, cam=None):
    """The scene's curvature constant as the library's own setup computes it (tests/raster_host: the same fill_uniforms)."""
    host = RasterScene(raster_lib(), dem, kw, cam=cam)
    try:
        assert host.curvature_enabled
        return host.inv_two_r_prime
    finally:
        host.close()


@pytest.fixture(scope="module")
def world():
    """The scenes and the sets with the reference's answers: computed once, shared, never written."""
    made = SimpleNamespace(scenes={}, sets={}, rasters={}, kw={}, cam={})
    heights, kw, rays = proof_scene()
    made.scenes["proof"] = describe(heights, kw, _constants(heights, kw, PROOF_CAM))
    made.sets["proof"] = TraceSet("proof", made.scenes["proof"], rays)
    made.kw["proof"], made.cam["proof"] = kw, PROOF_CAM
    for i, name in enumerate(SHAPES):
        dem, kw = shape_scene(name)
        scene = describe(dem, kw, _constants(dem, kw))
        made.scenes[name], made.kw[name], made.cam[name] = scene, kw, scenes.CAM
        made.sets[name] = TraceSet(f"list-{name}", scene, list_rays(scene, seed=4100 + i))
        if name in RASTER_SHAPES:
            made.rasters[name] = TraceSet(f"raster-{name}", scene, raster_rays(scene, False), raster=True, rays_curved=raster_rays(scene, True))
    return made


# ---- ray lists -----------------------------------------------------------------------------------------------------------------
def ground_gate(s, scene, what, n=1000, seed=99):
    """|top - t - bilinear_f64| <= 8 ulp(top): each of the two subtractions rounds once at the magnitude of top (4 ulp recorded on
    the golden DEM), the factor 2 covers a DEM with more relief."""
    surface = scene.surface
    rng = np.random.default_rng(seed)
    xz = np.stack([rng.uniform(surface.X[0], surface.X[-1], n), rng.uniform(surface.Z[0], surface.Z[-1], n)], 1).astype(f32)
    inside = (xz[:, 0] > surface.X[0]) & (xz[:, 0] < surface.X[-1]) & (xz[:, 1] > surface.Z[0]) & (xz[:, 1] < surface.Z[-1])
    xz = xz[inside]
    y = s.ground(xz)
    top = f32(float(scene.dem.max()) * scene.kw["exaggeration"] + s.GROUND_CLEARANCE)
    err = np.abs(y.astype(f64) - surface.height(xz[:, 0].astype(f64), xz[:, 1].astype(f64)))
    print(f"trace-ref {what} ground: {len(xz)} points, max |top - t - bilinear_f64| = {err.max():.3g} = {err.max() / float(np.spacing(top)):.2f} ulp(top = {float(top):g})")
    assert y.dtype == f32 and np.isfinite(y).all(), "inside the footprint there is ground"
    assert err.max() <= 8 * float(np.spacing(top))


@pytest.mark.parametrize("name", ["proof"] + list(SHAPES))
def test_trace_occluded_and_ground(world, name):
    ts = world.sets[name]
    with _session(ts.scene.dem, world.kw[name], world.cam[name]) as s:
        got = s.trace(ts.rays[False])
        assert not (got["kind"] == 2).any()
        gate_closest(ts, got["kind"] == 1, got["t"], got["normal"], "device trace")
        for curved in (False, True):
            gate_occlusion(ts, curved, s.occluded(ts.rays[curved], curved=curved), f"device occluded curved={curved}")
        ground_gate(s, ts.scene, ts.name)


# ---- rasters -------------------------------------------------------------------------------------------------------------------
def _host_form(s, curved, **kw):
    return lambda mode, targets, lift: s.visibility(targets, toward=mode == TOWARD, curved=curved, lift=lift, **kw)


def _tensor_form(s, curved):
    import torch

    def run(mode, targets, lift):
        d = torch.from_numpy(np.ascontiguousarray(targets, f32)).cuda()
        masks = s.visibility(d, toward=mode == TOWARD, curved=curved, lift=lift)
        assert masks.is_cuda and masks.dtype == torch.bool
        return masks.cpu().numpy()

    return run


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("name", RASTER_SHAPES)
def test_rasters(world, name, curved):
    ts = world.rasters[name]
    scene = ts.scene
    with _session(scene.dem, world.kw[name]) as s:
        lit = raster_bits(scene, _host_form(s, curved), curved)
        gate_occlusion(ts, curved, ~lit, f"device visibility, host form, curved={curved}")
        lit = raster_bits(scene, _tensor_form(s, curved), curved)
        gate_occlusion(ts, curved, ~lit, f"device visibility, tensor form, curved={curved}")
        # the wrappers are visibility at lift SURFACE_BIAS = 1e-3: the same bits as the gated call, through their own arguments
        assert f32(s.SURFACE_BIAS) == f32(LIFTS[1])
        observers, _ = viewshed_targets(scene, 2)
        seen = s.visibility(observers, toward=True, curved=curved, lift=LIFTS[1])
        for k, obs in enumerate(observers):
            one = s.viewshed(obs[:3], target_height=0.0, max_distance=float(obs[3]) if obs[3] > 0 else None, curved=curved)
            assert np.array_equal(one, seen[k]), f"viewshed of observer {k}"
        suns = np.stack([sun_direction(az, el) for az, el in SUNS])
        masks = s.visibility(suns, toward=False, curved=curved, lift=LIFTS[1])
        for k, sun in enumerate(suns):
            assert np.array_equal(s.shadow_mask(sun[:3], curved=curved), masks[k]), f"shadow_mask of sun {k}"
        hours = s.sun_hours(suns[:, :3], curved=curved)
        assert hours.dtype == np.uint32 and np.array_equal(hours, masks.sum(0)), "sun_hours equals the sum of the masks"


def test_a_strip_session_answers_the_whole_dem_as_the_reference(world):
    ts = world.rasters["63x65"]
    with _session(ts.scene.dem, world.kw["63x65"], row_begin=16, row_end=40) as s:
        for curved in (False, True):
            gate_occlusion(ts, curved, ~raster_bits(ts.scene, _host_form(s, curved), curved), f"strip session curved={curved}")
        lists = world.sets["63x65"]
        got = s.trace(lists.rays[False])
        gate_closest(lists, got["kind"] == 1, got["t"], got["normal"], "strip session trace")


# ---- the retable path -----------------------------------------------------------------------------------------------------------
def test_after_reterrain_the_reference_over_the_new_heights(world):
    dem, patch, result = reterrain_case()
    kw = world.kw["64x64"]
    scene = describe(result, kw, world.scenes["64x64"].inv_two_r_prime)
    lists = TraceSet("list-64x64-reterrain", scene, list_rays(scene, seed=4242))
    rasters = TraceSet("raster-64x64-reterrain", scene, raster_rays(scene, True), raster=True, which=(True,))
    with _session(dem, kw) as s:
        before = s.visibility(np.stack([sun_direction(az, el) for az, el in SUNS]), toward=False, lift=LIFTS[1])
        s.reterrain(patch, at=(20, 20))  # (nothing between the update and the queries)
        lit = raster_bits(scene, _host_form(s, True), True)
        got = s.trace(lists.rays[False])
        occluded = s.occluded(lists.rays[True], curved=True)
        after = s.visibility(np.stack([sun_direction(az, el) for az, el in SUNS]), toward=False, lift=LIFTS[1])
    gate_occlusion(rasters, True, ~lit, "after reterrain, visibility curved=True")
    gate_closest(lists, got["kind"] == 1, got["t"], got["normal"], "after reterrain, trace")
    gate_occlusion(lists, True, occluded, "after reterrain, occluded curved=True")
    assert (before != after).any(), "the patch changes what is lit"


# ---- the box city ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def city(world):
    dem, verts, tris, kw = city_scene()
    assert np.array_equal(world.scenes["64x64"].dem, dem)
    return dem, kw, CitySets(world.scenes["64x64"], verts, tris)


@pytest.mark.parametrize("mesh_builder", [0, 2, 3])
def test_city_against_terrain_or_triangles(city, mesh_builder):
    dem, kw, sets = city
    with _session(dem, kw, mesh_builder=mesh_builder) as s:
        for curved in (False, True):
            for terrain_only in (False, True):
                what = f"builder {mesh_builder} curved={curved} terrain_only={terrain_only}"
                got = s.occluded(sets.list.rays[curved], curved=curved, terrain_only=terrain_only)
                gate_city(sets.list, sets.mesh["list-64x64", curved], curved, got, terrain_only, f"city occluded {what}")
                lit = np.concatenate([s.visibility(targets, toward=mode == TOWARD, curved=curved, terrain_only=terrain_only, lift=LIFTS[1]).reshape(-1)
                                      for mode, targets in city_raster_targets(sets.raster.scene)])
                gate_city(sets.raster, sets.mesh["raster-city", curved], curved, ~lit, terrain_only, f"city visibility {what}")


# ---- the reference's curved-earth golden -------------------------------------------------------------------------------------------
def test_whitebox_curved_viewshed_equals_the_f64_reference():
    golden = whitebox_reference()
    dem, kw = whitebox_scene_kwargs()
    cam = {**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)}
    scene = describe(dem, kw, _constants(dem, kw, cam))
    obs = whitebox_observer(scene.origin, scene.spacing)
    o = contract_origins(dem, kw["exaggeration"], scene.origin, scene.spacing, (0, 0, *dem.shape), f32(1e-3))
    rays, go = contract_rays(o, TOWARD, obs[0], True, scene.inv_two_r_prime, True)
    assert go.all()
    ts = TraceSet("raster-whitebox", scene, rays, raster=True, which=(True,))  # (the flat DEM has no relief: the band is empty)
    with _session(dem, kw, cam=cam) as s:
        curved = s.viewshed(obs[0, :3], curved=True)
    gate_occlusion(ts, True, ~curved.reshape(-1), "device viewshed curved=True")
    reference = (ts.ref[True]["clear"] > 0.0).reshape(dem.shape)
    print(f"whitebox golden: the f64 reference's own IoU {iou(reference, golden):.5f} ({int(reference.sum())} visible, "
          f"{int((reference ^ golden).sum())} flipped), the device's {iou(curved, golden):.5f}")
    assert iou(curved, golden) >= 0.98
