"""DEM visibility rasters on a live terrain session (f3d_session_raster), the parts that need no GPU.

The lane body of the raster kernel (csrc/f3d_raster.h raster_origin / raster_visible, what k_raster runs per lane) compiled
for the host (tests/raster_host) and run over whole 64-lane waves -- the emulator's fibers, votes exchanged in lockstep, a
wave owning 64 consecutive samples of the region -- against ``oracle.terrain_trace_batch(any_hit=True)`` fed rays this file
builds in NumPy from the contract (`contract_rays`): f32, one rounding per operation, plane_at's single rounding through f64.
Every bit must be equal; nothing is left out.

* DEMs 5x3, 33x33, 64x64 and 65x63 (N no multiple of 64, waves that span rows), both target kinds, curved on and off,
  K = 1, 2, 3, a distance limit that cuts part of the raster, an observer exactly on a lifted sample, regions with nonzero
  row0 / col0 and a 1x1 region, NaN targets (the device form's path) answered 0 without a march;
* pad bits are zero, count equals masks.sum(0), the origins are the lifted lattice points;
* the reference's ridge and continuous-leaf cases, and its own curved-earth golden (IoU >= 0.98, flat control below);
* the header, the ctypes table and the descriptor's layout; the wrapper's methods.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scenes
from emul import emul
from oracle import oracle
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "raster_host" / "raster_harness.cpp"
GOLDEN = ROOT / "tests" / "golden" / "viewshed" / "whitebox_curved_analytic_256.png"
SIZE = (96, 64)
TOWARD, ALONG = 0, 1
TERRAIN_ONLY, CURVED, SESSION_SUN = 1, 2, 16
f32 = np.float32


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "raster_host")
    lib.raster_scene_create.restype = C.c_void_p
    lib.raster_scene_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.raster_scene_destroy.argtypes = [C.c_void_p]
    lib.raster_run.restype = C.c_int
    lib.raster_run.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_float, C.c_uint32] + [C.c_void_p] * 5
    lib.raster_desc_size.restype = C.c_uint32
    return lib


def _kw(dem, **extra):
    return scenes.fixed_frames(scenes.scene_kwargs(dem), 2, spp=1, earth_model="ellipsoid", refraction_model="bennett", **extra)


def unpack(words, n, rows, cols):
    """(K, ceil(n / 64)) uint64 -> bool (K, rows, cols); the pad bits must be zero."""
    words = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    assert not bits[:, n:].any(), "pad bits are zero"
    return bits[:, :n].astype(bool).reshape(words.shape[0], rows, cols)


class HostScene:
    """A scene as the emulator sets it up, and rasters over it as f3d_session_raster's device form answers them."""

    def __init__(self, lib, dem, kw, cam=None, mesh_form=2):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        d, keep = _desc(self.dem, SIZE, cam or scenes.CAM, kw)
        info = np.zeros(9, f32)
        self.handle = lib.raster_scene_create(C.addressof(d), mesh_form, info.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin = (f32(info[0]), f32(info[1]))
        self.spacing = (f32(info[2]), f32(info[3]))
        self.inv_two_r_prime, self.curvature_enabled = f32(info[4]), bool(info[5])
        self.sun = info[6:9].copy()

    def close(self):
        self.lib.raster_scene_destroy(self.handle)

    def region(self, region):
        return (0, 0, *self.dem.shape) if region is None else tuple(int(v) for v in region)

    def run(self, mode, targets, flags=0, region=None, lift=0.0):
        row0, col0, rows, cols = self.region(region)
        n = rows * cols
        if flags & SESSION_SUN:
            k, ptr = 1, None
        else:
            targets = np.ascontiguousarray(targets, f32).reshape(-1, 4)
            k, ptr = len(targets), targets.ctypes.data
        masks = np.full((k, (n + 63) // 64), 0x7777777777777777, np.uint64)
        count = np.full(n, 77, np.uint32)
        marches = np.full((k, n), 77, np.uint32)
        origins = np.full((n, 3), 77, f32)
        assert self.lib.raster_run(self.handle, mode, flags, row0, col0, rows, cols, float(lift), k, ptr, masks.ctypes.data,
                                   count.ctypes.data, marches.ctypes.data, origins.ctypes.data) == 0
        return {"masks": unpack(masks, n, rows, cols), "count": count.reshape(rows, cols), "marches": marches.reshape(k, rows, cols),
                "origins": origins.reshape(rows, cols, 3)}


# ---- the contract, restated in NumPy -----------------------------------------------------------------------------------------
def plane_at(origin, index, spacing):
    """f3d_trace.h plane_at: fma(f32(index), spacing, origin) -- the product is exact in f64, the sum rounded once."""
    return (index.astype(np.float64) * np.float64(spacing) + np.float64(origin)).astype(f32)


def contract_origins(dem, exaggeration, origin, spacing, region, lift):
    """(rows, cols, 3) f32: the lifted lattice points of the region."""
    row0, col0, rows, cols = region
    j, i = np.meshgrid(np.arange(row0, row0 + rows), np.arange(col0, col0 + cols), indexing="ij")
    h = np.asarray(dem, f32) * f32(exaggeration)  # (the sample as the session holds it)
    return np.stack([plane_at(origin[0], i, spacing[0]), h[j, i] + f32(lift), plane_at(origin[1], j, spacing[1])], -1).astype(f32)


def contract_rays(o, mode, target, curved, inv_two_r_prime, curvature_enabled):
    """One target over the origins o (..., 3): rays (n, 8) f32 and `go` (n,) -- False: cut off by the distance limit or a ray
    query_ray_good refuses, answered 0 without a march."""
    o = o.reshape(-1, 3)
    x, y, z, w = (f32(v) for v in target)
    with np.errstate(all="ignore"):
        if mode == TOWARD:
            dx, dz = x - o[:, 0], z - o[:, 2]
            hd2 = dx * dx + dz * dz
            dy = y - o[:, 1]
            if curved and curvature_enabled:
                dy = dy - hd2 * f32(inv_two_r_prime)
            d = np.stack([dx, dy, dz], 1).astype(f32)
            tmax = f32(1.0)
            go = ~((w > 0) & (hd2 > w * w))
        else:
            d = np.broadcast_to(np.array([x, y, z], f32), o.shape).copy()
            tmax = f32(1e30)
            go = np.ones(len(o), bool)
        len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        go = go & np.isfinite(o).all(1) & np.isfinite(d).all(1) & (len2 > 0) & np.isfinite(len2)
    assert d.dtype == f32 and len2.dtype == f32
    rays = np.zeros((len(o), 8), f32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, tmax
    return rays, go


def contract_bits(scene, mode, targets, curved, region=None, lift=0.0, occluded=None):
    """Bool (K, rows, cols) the contract asks for.  `occluded(rays) -> bool (n,)` answers the rays that march: by default the
    oracle's terrain trace; a GPU test hands in the session's own occluded() where the scene has a mesh."""
    region = scene.region(region)
    o = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, region, lift)
    out = []
    for target in np.asarray(targets, f32).reshape(-1, 4):
        rays, go = contract_rays(o, mode, target, curved, scene.inv_two_r_prime, scene.curvature_enabled)
        bits = np.zeros(len(rays), bool)
        if go.any():
            if occluded is None:
                hit = oracle.terrain_trace_batch(scene.dem, rays[go], origin=tuple(float(v) for v in scene.origin),
                                                 spacing=tuple(float(v) for v in scene.spacing), exaggeration=scene.kw["exaggeration"],
                                                 inv_two_r_prime=float(scene.inv_two_r_prime), curvature_enabled=scene.curvature_enabled,
                                                 any_hit=True, apply_curvature=curved)["hit"] != 0
            else:
                hit = np.asarray(occluded(rays[go]), bool)
            bits[go] = ~hit
        out.append(bits.reshape(region[2], region[3]))
    return np.stack(out)


def sun_direction(azimuth_deg, elevation_deg):
    az, el = np.radians(azimuth_deg), np.radians(elevation_deg)
    return np.array([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el), 0.0], f32)


# ---- the shapes where it can go wrong -------------------------------------------------------------------------------------
def shaped_dem(shape):
    """The golden DEM's relief on a grid of `shape` (rows, cols): its 64x64 samples, cropped / tiled."""
    g = scenes.golden_dem(4)
    assert g.shape == (64, 64)
    rows, cols = shape
    return np.ascontiguousarray(np.pad(g, ((0, max(rows - 64, 0)), (0, max(cols - 64, 0))), mode="reflect")[:rows, :cols])


SHAPES = [(3, 5), (33, 33), (64, 64), (63, 65)]  # 5x3, 33x33, 64x64, 65x63 as width x height


@pytest.fixture(scope="module")
def shaped(harness):
    made = {}
    for shape in SHAPES:
        dem = shaped_dem(shape)
        made[shape] = HostScene(harness, dem, _kw(dem))
    yield made
    for s in made.values():
        s.close()


def viewshed_targets(scene, k=3, lift=0.5):
    """K observers over the scene: one high over the footprint (the issue's (0.3 ox, 16, 0.2 ox)), one with a distance limit that
    cuts part of the raster, one standing EXACTLY on a lifted sample (its own ray has a zero direction)."""
    ox = float(scene.origin[0])
    rows, cols = scene.dem.shape
    span = float(scene.spacing[0]) * (cols - 1)
    on = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, (rows // 2, cols // 3, 1, 1), lift)[0, 0]
    t = np.array([[0.3 * ox, 16.0, 0.2 * ox, 0.0],
                  [-0.2 * ox, 18.0, 0.1 * ox, 0.35 * span],
                  [on[0], on[1], on[2], 0.0]], f32)
    return t[:k], (rows // 2, cols // 3)


def sun_targets(k=3):
    return np.stack([sun_direction(315.0, el) for el in (5.0, 15.0, 30.0)])[:k]


def _check(scene, mode, targets, curved, region=None, lift=0.0, flags=0):
    got = scene.run(mode, targets, flags=flags | (CURVED if curved else 0), region=region, lift=lift)
    want = contract_bits(scene, mode, targets, curved, region, lift)
    wrong = int((got["masks"] != want).sum())
    assert wrong == 0, f"{wrong} of {want.size} bits differ from the oracle"
    assert np.array_equal(got["count"], want.sum(0).astype(np.uint32)), "count equals masks.sum(0)"
    return got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_origins_are_the_lifted_lattice_points(shaped, shape):
    scene = shaped[shape]
    for region, lift in ((None, 0.0), (None, 1e-3), ((1, 2, 2, 3), 0.5)):
        got = scene.run(ALONG, sun_targets(1), region=region, lift=lift)["origins"]
        want = contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, scene.region(region), lift)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_viewshed_equals_the_oracle_bit_for_bit(shaped, shape, curved):
    scene = shaped[shape]
    assert scene.curvature_enabled and scene.inv_two_r_prime > 0.0
    targets, on = viewshed_targets(scene)
    got, want = _check(scene, TOWARD, targets, curved, lift=0.5)
    if shape[0] * shape[1] > 64:
        assert want[0].any() and not want[0].all(), "both answers occur"
        rays, go = contract_rays(contract_origins(scene.dem, scene.kw["exaggeration"], scene.origin, scene.spacing, scene.region(None), 0.5),
                                 TOWARD, targets[1], curved, scene.inv_two_r_prime, scene.curvature_enabled)
        assert go.any() and not go.all(), "the distance limit cuts part of the raster"
        assert not got["masks"][1].reshape(-1)[~go].any() and not got["marches"][1].reshape(-1)[~go].any(), "cut off: 0, and no march"
    assert not got["masks"][2][on] and got["marches"][2][on] == 0, "the observer's own sample: a zero direction, answered 0 unmarched"
    assert (got["marches"][0] >= 1).all()


@pytest.mark.parametrize("curved", [False, True], ids=["flat", "curved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_sun_mask_equals_the_oracle_bit_for_bit(shaped, shape, curved):
    scene = shaped[shape]
    got, want = _check(scene, ALONG, sun_targets(), curved, lift=1e-3)
    if shape[0] * shape[1] > 64:
        assert want[0].any() and not want[0].all(), "both answers occur at elevation 5"
        assert want[0].sum() < want[2].sum(), "a higher sun lights more"


@pytest.mark.parametrize("k", [1, 2, 3])
def test_target_counts(shaped, k):
    scene = shaped[(63, 65)]
    _check(scene, TOWARD, viewshed_targets(scene, k)[0], False, lift=0.5)
    got, _ = _check(scene, ALONG, sun_targets(k), True, lift=1e-3)
    assert got["masks"].shape == (k, 63, 65) and int(got["count"].max()) <= k


@pytest.mark.parametrize("region", [(1, 2, 2, 3), (7, 5, 40, 33), (62, 64, 1, 1), (0, 64, 63, 1), (31, 0, 1, 65), (20, 20, 1, 1)])
def test_regions(shaped, region):
    scene = shaped[(63, 65)]
    whole = contract_bits(scene, TOWARD, viewshed_targets(scene)[0], True, None, 0.5)
    got, want = _check(scene, TOWARD, viewshed_targets(scene)[0], True, region=region, lift=0.5)
    r0, c0, r, c = region
    assert np.array_equal(want, whole[:, r0:r0 + r, c0:c0 + c]), "a region is a window of the whole raster"
    _check(scene, ALONG, sun_targets(), False, region=region, lift=1e-3)


def test_session_sun_is_the_armed_direction(shaped):
    scene = shaped[(64, 64)]
    target = np.array([[*scene.sun, 0.0]], f32)
    for curved in (False, True):
        sun = scene.run(ALONG, None, flags=SESSION_SUN | (CURVED if curved else 0), lift=1e-3)
        given, _ = _check(scene, ALONG, target, curved, lift=1e-3)
        assert np.array_equal(sun["masks"], given["masks"]) and np.array_equal(sun["count"], given["count"])
        assert sun["masks"].any() and not sun["masks"].all()


def test_nan_targets_answer_zero_and_are_never_marched(shaped):
    """The device form's path: the host never sees the targets, the lanes refuse the rays."""
    scene = shaped[(63, 65)]
    good, _ = viewshed_targets(scene)
    for mode, base in ((TOWARD, good[0]), (ALONG, sun_targets(1)[0])):
        for slot in range(3):
            for value in (np.nan, np.inf, -np.inf):
                bad = base.copy()
                bad[slot] = value
                targets = np.stack([base, bad, base])
                got = scene.run(mode, targets, flags=CURVED, lift=0.5)
                assert not got["masks"][1].any() and not got["marches"][1].any(), (mode, slot, value)
                assert np.array_equal(got["masks"][0], got["masks"][2]) and got["masks"][0].any()
                assert np.array_equal(got["count"], got["masks"].sum(0))
    # a NaN distance limit is no limit (w > 0 fails); a zero direction is refused
    nolimit = good[0].copy()
    nolimit[3] = np.nan
    assert np.array_equal(scene.run(TOWARD, nolimit, lift=0.5)["masks"], scene.run(TOWARD, good[0], lift=0.5)["masks"])
    zero = scene.run(ALONG, np.zeros(4, f32), lift=0.5)
    assert not zero["masks"].any() and not zero["marches"].any()


def test_terrain_only_and_mesh_forms_agree_without_a_mesh_and_differ_with_one(harness):
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    kw = _kw(dem, mesh_vertices=verts, mesh_indices=tris)
    forms = [HostScene(harness, dem, kw, mesh_form=f) for f in (0, 1, 2)]
    try:
        targets = sun_targets()
        runs = [s.run(ALONG, targets, flags=CURVED, lift=1e-3) for s in forms]
        assert all(np.array_equal(runs[0]["masks"], r["masks"]) for r in runs[1:]), "the answers do not depend on the tree's form"
        bare = forms[2].run(ALONG, targets, flags=CURVED | TERRAIN_ONLY, lift=1e-3)
        want = contract_bits(forms[2], ALONG, targets, True, None, 1e-3)
        assert np.array_equal(bare["masks"], want), "TERRAIN_ONLY: the oracle's terrain answer"
        assert not (runs[2]["masks"] & ~bare["masks"]).any() and (runs[2]["masks"] != bare["masks"]).any(), "the boxes only ever shade"
    finally:
        for s in forms:
            s.close()


# ---- inputs with known answers -----------------------------------------------------------------------------------------------
def test_golden_dem_fractions(shaped):
    """The golden DEM at exaggeration 20: the observer (0.3 ox, 16, 0.2 ox) sees 69 % of the samples, the sun at azimuth 315
    lights 43.6 / 78.8 / 94.4 % at elevation 5 / 15 / 30 (measured on the oracle): both answers occur."""
    scene = shaped[(64, 64)]
    assert scene.kw["exaggeration"] == 20.0
    ox = float(scene.origin[0])
    got, _ = _check(scene, TOWARD, np.array([[0.3 * ox, 16.0, 0.2 * ox, 0.0]], f32), False, lift=1e-3)
    seen = got["masks"].mean()
    lit = [_check(scene, ALONG, sun_direction(315.0, el), True, lift=1e-3)[0]["masks"].mean() for el in (5.0, 15.0, 30.0)]
    print(f"golden DEM: visible {100 * seen:.1f} %, lit at elevation 5 / 15 / 30: " + " / ".join(f"{100 * v:.1f} %" for v in lit))
    assert round(100 * seen) == 69 and [round(1000 * v) for v in lit] == [436, 788, 944]


def _planar(dem, spacing):
    kw = _kw(dem)
    kw.update(spacing=(spacing, spacing), exaggeration=1.0)
    return kw


def test_ridge_case(harness):
    """The reference's ridge: 33x33, column 16 at 600 m, 3 400 m cells, the observer 100 m up at column 3.2 of row 16.  Behind
    the ridge nothing is seen; the curvature hides the far ground in front of it too."""
    dem = np.zeros((33, 33), f32)
    dem[:, 16] = 600.0
    scene = HostScene(harness, dem, _planar(dem, 3400.0), cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        assert scene.curvature_enabled
        obs = np.array([[float(scene.origin[0]) + 3.2 * 3400.0, 100.0, float(scene.origin[1]) + 16 * 3400.0, 0.0]], f32)
        flat, _ = _check(scene, TOWARD, obs, False, lift=1e-3)
        curved, _ = _check(scene, TOWARD, obs, True, lift=1e-3)
        print(f"ridge: {int(flat['masks'].sum())} samples visible flat, {int(curved['masks'].sum())} curved")
        assert flat["masks"][0, 16, 10] and not flat["masks"][0, 16, 24]
        assert not flat["masks"][0][:, 17:].any(), "nothing behind the ridge"
        assert flat["masks"][0][:, :16].all(), "flat ground in front of the ridge is in plain sight"
        assert int(flat["masks"].sum()) == 561 and int(curved["masks"].sum()) == 318 and not (curved["masks"] & ~flat["masks"]).any()
    finally:
        scene.close()


def test_continuous_leaf_case(harness):
    """The reference's continuous_leaf patch [[16.5, 28.5], [28.5, 24.5]]: from 25 over sample (0, 0), sample (1, 1) lifted by 0.5
    to the same height lies behind the saddle's flank (25.5 at three quarters of the diagonal): blocked.  The linear
    interpolation of the corners along that diagonal would see it."""
    dem = np.array([[16.5, 28.5], [28.5, 24.5]], f32)
    scene = HostScene(harness, dem, _planar(dem, 1.0))
    try:
        obs = np.array([[scene.origin[0], 25.0, scene.origin[1], 0.0]], f32)
        got, _ = _check(scene, TOWARD, obs, False, lift=0.5)
        assert not got["masks"][0, 1, 1]
    finally:
        scene.close()


# ---- the reference's own curved-earth golden -----------------------------------------------------------------------------------
def whitebox_scene_kwargs():
    dem = np.zeros((256, 256), f32)
    kw = _kw(dem)
    kw.update(spacing=(434.8, 431.9), exaggeration=1.0, earth_model="ellipsoid", refraction_model="effective_radius", refraction_k=0.13,
              observer_latitude_deg=0.0)
    return dem, kw


def whitebox_reference():
    from PIL import Image

    image = np.array(Image.open(GOLDEN))
    return (image[..., 0] if image.ndim == 3 else image) > 0


def whitebox_observer(origin, spacing):
    return np.array([[plane_at(origin[0], np.array(127), spacing[0]), 250.0, plane_at(origin[1], np.array(127), spacing[1]), 0.0]], f32)


def iou(a, b):
    return float((a & b).sum()) / float((a | b).sum())


def test_whitebox_curved_golden_on_the_host_body(harness):
    """The reference's gate on its committed analytic curved-earth viewshed: IoU >= 0.98 curved, the flat control below 0.98."""
    reference = whitebox_reference()
    assert reference.shape == (256, 256) and int(reference.sum()) == 57_957
    dem, kw = whitebox_scene_kwargs()
    scene = HostScene(harness, dem, kw, cam={**scenes.CAM, "origin": (0.0, 9000.0, 90000.0)})
    try:
        obs = whitebox_observer(scene.origin, scene.spacing)
        curved = scene.run(TOWARD, obs, flags=CURVED, lift=1e-3)["masks"][0]
        flat = scene.run(TOWARD, obs, lift=1e-3)["masks"][0]
        print(f"whitebox golden: curved IoU {iou(curved, reference):.5f} ({int(curved.sum())} visible, {int((curved ^ reference).sum())} flipped), "
              f"flat control {iou(flat, reference):.7f}")
        assert iou(curved, reference) >= 0.98
        assert iou(flat, reference) < 0.98
    finally:
        scene.close()


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_layout(harness):
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header, "the raster is additive: no ABI version bump"
    body = re.search(r"typedef struct f3d_session_raster_desc \{(.*?)\} f3d_session_raster_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [name for name, _ in _native.RasterDesc._fields_]
    assert members == ["struct_size", "mode", "flags", "row0", "col0", "rows", "cols", "lift", "target_count", "reserved", "targets", "masks",
                       "count"]
    assert C.sizeof(_native.RasterDesc) == 40 + 3 * 8 == harness.raster_desc_size()
    assert _native.RasterDesc.targets.offset == 40 and _native.RasterDesc.lift.offset == 28
    assert re.search(r"int f3d_session_raster\(f3d_session \*session, const f3d_session_raster_desc \*desc, char \*err, size_t errlen\);", header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_raster"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for name, value in (("TOWARD_POINT", 0), ("ALONG_DIRECTION", 1), ("TERRAIN_ONLY", 1), ("CURVED", 2), ("DEVICE_POINTERS", 4), ("NO_WAIT", 8),
                        ("SESSION_SUN", 16)):
        assert re.search(rf"#define F3D_RASTER_{name} {value}u", header) and getattr(_native, f"RASTER_{name}") == value


def test_wrapper_has_the_raster_methods():
    import inspect

    from forge3d_amd.session import TerrainSession

    for name in ("visibility", "viewshed", "shadow_mask", "sun_hours"):
        assert callable(getattr(TerrainSession, name))
    p = inspect.signature(TerrainSession.viewshed).parameters
    assert p["observer_height"].default == 1.7 and p["target_height"].default == 0.0 and p["max_distance"].default is None
    assert p["curved"].default is False and inspect.signature(TerrainSession.shadow_mask).parameters["curved"].default is True
    assert inspect.signature(TerrainSession.shadow_mask).parameters["direction"].default is None
