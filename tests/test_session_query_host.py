"""Ray queries on a live terrain session (f3d_session_query), the parts that need no GPU.

The lane body of the query kernel (csrc/f3d_query.h query_lane, what k_query runs per lane) compiled for the host
(tests/query_host) and run over whole 64-lane waves -- the emulator's fibers, votes exchanged in lockstep:

* terrain against the oracle bit for bit: the reference's proof rays over its 256^2 proof DEM (closest hit: hit, t, normal;
  occlusion with and without the curvature policy: the hit bits) and 4 000 vertical "ground" rays over the golden DEM,
  lattice points and borders included (top - t equals the oracle's);
* mesh: the pixel query over a whole 96x64 view of the box city equals the oracle's depth and normal AOVs, `kind` is 2
  exactly where the albedo AOV is the mesh's, the three tree forms (sweep, binary, four wide) answer identically, the
  closest-hit query fed the pixel query's directions returns the pixel query's answers;
* `primitive`: the mesh triangle is the nearest one of an f64 brute-force Moeller-Trumbore search (ties apart), the terrain
  cell holds the hit position;
* bad rays (NaN / +-inf in every slot, zero direction, tmax <= tmin) mixed into waves of good ones: a miss, the good ones
  unchanged, and no march entered for them;
* the header, the ctypes table and the descriptor's layout.
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
from trace_reference import triangle_search

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "query_host" / "query_harness.cpp"
QNAN = 0x7FC00000
NONE = 0xFFFFFFFF
SIZE = (96, 64)


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "query_host")
    lib.query_scene_create.restype = C.c_void_p
    lib.query_scene_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.query_scene_destroy.argtypes = [C.c_void_p]
    lib.query_run.restype = C.c_int
    lib.query_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8
    return lib


class HostScene:
    """A scene as the emulator sets it up, and query batches over it as f3d_session_query answers them."""

    def __init__(self, lib, dem, cam, kw, mesh_form=2):
        self.lib = lib
        d, keep = _desc(dem, SIZE, cam, kw)
        info = np.zeros(4, np.float32)
        self.handle = lib.query_scene_create(C.addressof(d), mesh_form, info.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin = (np.float32(info[0]), np.float32(info[1]))
        self.inv_two_r_prime, self.curvature_enabled = float(info[2]), bool(info[3])

    def close(self):
        self.lib.query_scene_destroy(self.handle)

    def run(self, mode, rays, flags=0):
        rays = np.ascontiguousarray(rays, np.uint32 if mode == 2 else np.float32)
        n = rays.shape[0]
        out = {"kind": np.full(n, 77, np.uint32), "marches": np.full(n, 77, np.uint32)}
        if mode != 1:
            out.update(t=np.full(n, 77, np.float32), normal=np.full((n, 3), 77, np.float32), position=np.full((n, 3), 77, np.float32),
                       primitive=np.full(n, 77, np.uint32))
        if mode == 2:
            out["direction"] = np.full((n, 3), 77, np.float32)
        ptr = [out[k].ctypes.data if k in out else None for k in ("kind", "t", "normal", "position", "primitive", "direction", "marches")]
        assert self.lib.query_run(self.handle, mode, flags, n, rays.ctypes.data, *ptr) == 0
        return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]) if a[k].dtype == np.float32 else a[k], _bits(b[k]) if b[k].dtype == np.float32 else b[k])
               for k in a if k != "marches")


def _kw(dem, **extra):
    return scenes.fixed_frames(scenes.scene_kwargs(dem), 2, spp=1, earth_model="ellipsoid", refraction_model="bennett", **extra)


# ---- terrain against the oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proof(harness):
    heights, rays = scenes.proof_rays(n_random=2000, mask=False)
    kw = dict(_kw(heights), spacing=(500.0, 500.0), exaggeration=1.0)
    cam = {"origin": (0.0, 9000.0, 90000.0), "look_at": (0.0, 900.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 45.0, "exposure": 1.0}
    scene = HostScene(harness, heights, cam, kw)
    rays = rays.copy()  # the session centres the DEM: the rays move with it, in f32
    rays[:, 0] += scene.origin[0]
    rays[:, 2] += scene.origin[1]
    yield scene, heights, rays
    scene.close()


def _oracle_batch(scene, heights, rays, spacing, exaggeration, **kw):
    return oracle.terrain_trace_batch(heights, rays, origin=tuple(float(v) for v in scene.origin), spacing=(spacing, spacing),
                                      exaggeration=exaggeration, inv_two_r_prime=scene.inv_two_r_prime,
                                      curvature_enabled=scene.curvature_enabled, **kw)


def test_closest_hit_equals_the_oracle_bit_for_bit(proof):
    scene, heights, rays = proof
    got = scene.run(0, rays)
    want = _oracle_batch(scene, heights, rays, 500.0, 1.0, any_hit=False, apply_curvature=False)
    hit = want["hit"] != 0
    assert 50 < hit.sum() < len(rays) - 50, "the proof rays hit and miss"
    assert np.array_equal(got["kind"], hit.astype(np.uint32))  # (no mesh: a hit is terrain)
    assert np.array_equal(_bits(got["t"])[hit], _bits(want["t"])[hit])
    assert np.array_equal(_bits(got["normal"])[hit], _bits(want["normal"])[hit])
    assert np.all(_bits(got["t"])[~hit] == QNAN) and not got["normal"][~hit].any() and not got["position"][~hit].any()
    assert np.all(got["primitive"][~hit] == NONE)


@pytest.mark.parametrize("curved", [False, True])
def test_occlusion_equals_the_oracle(proof, curved):
    scene, heights, rays = proof
    assert scene.curvature_enabled and scene.inv_two_r_prime > 0.0
    got = scene.run(1, rays, flags=2 if curved else 0)
    want = _oracle_batch(scene, heights, rays, 500.0, 1.0, any_hit=True, apply_curvature=curved)
    assert np.array_equal(got["kind"], (want["hit"] != 0).astype(np.uint32))
    assert 50 < got["kind"].sum() < len(rays) - 50


def test_curvature_policy_changes_occlusion_answers(proof):
    scene, _, rays = proof
    assert (scene.run(1, rays)["kind"] != scene.run(1, rays, flags=2)["kind"]).any()


def _ground_points(dem, spacing, n=4000, seed=20250):
    """(n, 2) f32 (x, z): random points of the footprint, lattice points, the four borders, a few outside."""
    h, w = dem.shape
    ox, oz = np.float32(-0.5 * (w - 1.0) * spacing), np.float32(-0.5 * (h - 1.0) * spacing)
    rng = np.random.default_rng(seed)
    inner = np.stack([rng.uniform(ox, -ox, n - 700), rng.uniform(oz, -oz, n - 700)], 1).astype(np.float32)
    ij = rng.integers(0, [w, h], (400, 2))
    lattice = np.stack([ox + ij[:, 0].astype(np.float32) * np.float32(spacing), oz + ij[:, 1].astype(np.float32) * np.float32(spacing)], 1)
    u = rng.uniform(ox, -ox, 50).astype(np.float32)
    border = np.concatenate([np.stack([u, np.full(50, oz)], 1), np.stack([u, np.full(50, -oz)], 1),
                             np.stack([np.full(50, ox), u], 1), np.stack([np.full(50, -ox), u], 1)]).astype(np.float32)
    outside = np.stack([rng.uniform(1.01, 2.0, 100) * rng.choice([-1.0, 1.0], 100) * float(-ox), rng.uniform(oz, -oz, 100)], 1).astype(np.float32)
    return np.concatenate([inner, lattice, border, outside]).astype(np.float32), len(inner)


def test_ground_equals_the_oracle_bit_for_bit(harness):
    """top - t of 4 000 vertical rays from top = max * exaggeration + 10 equals the oracle's, bit for bit; NaN outside the
    footprint.  Gated at 8 ulp(top): how far those heights are from the f64 bilinear patch (measured on the oracle: 7.2e-6 at
    relief 20, about 4 ulp of top = 30; the rounding of top - t, not of the intersection; the factor 2 is for more relief)."""
    dem = scenes.golden_dem(4)
    kw = _kw(dem)
    spacing = kw["spacing"][0]
    scene = HostScene(harness, dem, scenes.CAM, kw)
    try:
        xz, n_inner = _ground_points(dem, spacing)
        top = np.float32(float(dem.max()) * kw["exaggeration"] + 10.0)
        rays = np.zeros((len(xz), 8), np.float32)
        rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5], rays[:, 7] = xz[:, 0], top, xz[:, 1], -1.0, 1e30
        got = scene.run(0, rays, flags=1)
        want = _oracle_batch(scene, dem, rays, spacing, kw["exaggeration"], any_hit=False, apply_curvature=False)
        hit = want["hit"] != 0
        assert hit[:n_inner].all() and not hit[-100:].any(), "inside the footprint there is ground, outside none"
        assert np.array_equal(got["kind"], hit.astype(np.uint32))
        y_got, y_want = top - got["t"], top - want["t"]
        assert np.array_equal(_bits(y_got)[hit], _bits(y_want)[hit])
        assert np.isnan(y_got[~hit]).all()
        # the f64 bilinear patch under the inner points
        h, w = dem.shape
        fx = (xz[:n_inner, 0].astype(np.float64) - float(scene.origin[0])) / spacing
        fz = (xz[:n_inner, 1].astype(np.float64) - float(scene.origin[1])) / spacing
        i, j = np.clip(fx.astype(int), 0, w - 2), np.clip(fz.astype(int), 0, h - 2)
        a, b = fx - i, fz - j
        z = (dem.astype(np.float32) * np.float32(kw["exaggeration"])).astype(np.float64)
        ref = (z[j, i] * (1 - a) + z[j, i + 1] * a) * (1 - b) + (z[j + 1, i] * (1 - a) + z[j + 1, i + 1] * a) * b
        err = np.abs(y_got[:n_inner].astype(np.float64) - ref)
        print(f"ground: max |top - t - bilinear_f64| = {err.max():.3g} (top = {float(top):g}, ulp(top) = {float(np.spacing(top)):.3g})")
        assert err.max() <= 8 * float(np.spacing(top)), "each of the two subtractions rounds once at the magnitude of top"
    finally:
        scene.close()


# ---- mesh -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def city(harness):
    dem = scenes.golden_dem(4)
    verts, tris = scenes.box_city(n_boxes=30, seed=5)
    assert len(tris) == 385
    kw = _kw(dem, mesh_vertices=verts, mesh_indices=tris)
    scene_forms = [HostScene(harness, dem, scenes.CAM, kw, mesh_form=f) for f in (0, 1, 2)]
    want = oracle.render(dem, SIZE[0], SIZE[1], scenes.CAM, **kw)
    pixels = np.stack(np.meshgrid(np.arange(SIZE[0]), np.arange(SIZE[1])), -1).reshape(-1, 2).astype(np.uint32)
    picked = scene_forms[2].run(2, pixels)
    yield scene_forms, dem, verts, tris, want, pixels, picked
    for s in scene_forms:
        s.close()


def _half(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def test_pixel_query_equals_the_oracles_aovs(city):
    _, _, _, _, want, pixels, got = city
    n = len(pixels)
    assert n == 6144
    assert np.array_equal(_bits(got["t"]), _bits(want["depth"]).reshape(-1)), "depth AOV, qNaN on sky included"
    # the normal AOV is the G-buffer normal through RGBA16F (render_terrain.rs:1367-1393): compared at that precision
    assert np.array_equal(_bits(_half(got["normal"])), _bits(want["normal"]).reshape(-1, 3))
    mesh = np.all(_bits(want["albedo"]).reshape(-1, 3) == _bits(_half([0.7, 0.7, 0.8])), axis=1)
    assert np.array_equal(got["kind"] == 2, mesh)
    counts = (int((got["kind"] == 2).sum()), int((got["kind"] == 1).sum()), int((got["kind"] == 0).sum()))
    print("pixel query: mesh / terrain / sky pixels =", counts)
    assert counts == (1575, 2056, n - 1575 - 2056)
    sky = got["kind"] == 0
    assert np.all(got["primitive"][sky] == NONE) and not got["position"][sky].any() and not got["normal"][sky].any()
    assert np.all(np.abs(np.linalg.norm(got["direction"], axis=1) - 1.0) < 1e-6)


def _rays_of(picked):
    n = len(picked["kind"])
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = np.asarray(scenes.CAM["origin"], np.float32)
    rays[:, 3], rays[:, 4:7], rays[:, 7] = 1e-3, picked["direction"], 1e30
    return rays


def test_tree_forms_and_modes_agree(city):
    forms, _, _, _, _, pixels, picked = city
    rays = _rays_of(picked)
    closest = [s.run(0, rays) for s in forms]
    assert _same(closest[0], closest[1]) and _same(closest[0], closest[2]), "sweep, binary walk and four-wide walk answer identically"
    want = {k: v for k, v in picked.items() if k != "direction"}
    assert _same(want, closest[2]), "mode 0 fed mode 2's directions returns mode 2's answers"
    assert _same(picked, forms[0].run(2, pixels)) and _same(picked, forms[1].run(2, pixels))
    # occlusion: secondary rays from the hit points towards a low sun, and the camera rays themselves
    hit = picked["kind"] != 0
    sun = np.array([0.6, 0.3, -0.5], np.float32)
    shadow = np.zeros((int(hit.sum()), 8), np.float32)
    shadow[:, 0:3] = picked["position"][hit] + np.float32(1e-3) * picked["normal"][hit]
    shadow[:, 3], shadow[:, 4:7], shadow[:, 7] = 1e-3, sun, 1e30
    for batch in (shadow, rays):
        for flags in (0, 2):
            occ = [s.run(1, batch, flags=flags)["kind"] for s in forms]
            assert np.array_equal(occ[0], occ[1]) and np.array_equal(occ[0], occ[2])
    # (the reference's any-hit march is not its closest-hit march asked for existence: a handful of grazing camera rays are
    # "occluded" without a closest hit -- so the camera rays are compared with the oracle's any-hit batch, terrain only)
    _, dem, _, _, _, _, _ = city
    kw = scenes.scene_kwargs(dem)
    any_hit = _oracle_batch(forms[2], dem, rays, kw["spacing"][0], kw["exaggeration"], any_hit=True, apply_curvature=False)["hit"] != 0
    assert np.array_equal(forms[2].run(1, rays, flags=1)["kind"] != 0, any_hit)
    assert ((forms[2].run(1, rays)["kind"] != 0) == hit).mean() > 0.99
    blocked = forms[2].run(1, shadow)["kind"]
    assert 0 < blocked.sum() < len(blocked)


def test_terrain_only_leaves_the_mesh_out(city):
    forms, dem, _, _, _, pixels, picked = city
    bare = forms[2].run(2, pixels, flags=1)
    assert not (bare["kind"] == 2).any() and (bare["kind"][picked["kind"] == 2] == 1).sum() > 1000
    # a terrain hit in front of every triangle stays, a mesh hit gives way to what is behind it.  (Same cell, not always the
    # same bits: the reference marches the terrain with tmax = the mesh's hit, and a leaf cut by tmax is solved over the cut
    # interval -- the last bits of t may differ between the two queries.)
    same = picked["kind"] != 2
    assert np.array_equal(picked["kind"][same], bare["kind"][same]) and np.array_equal(picked["primitive"][same], bare["primitive"][same])
    ground = picked["kind"] == 1
    assert np.all(np.abs(picked["t"][ground] - bare["t"][ground]) <= 1e-5 * bare["t"][ground])
    assert _same(picked, bare) is False


def test_primitive_names_what_was_hit(city):
    forms, dem, verts, tris, _, _, picked = city
    # more mesh hits than the view has: rays from above aimed into the city as well
    rng = np.random.default_rng(11)
    extra = np.zeros((600, 8), np.float32)
    extra[:, 0:3] = rng.uniform([-60, 30, -60], [60, 70, 60], (600, 3))
    target = rng.uniform([-45, 0, -45], [45, 20, 45], (600, 3))
    extra[:, 3], extra[:, 4:7], extra[:, 7] = 1e-3, target - extra[:, 0:3], 1e30  # (unnormalised: t in units of |d|)
    rays = np.concatenate([_rays_of(picked), extra])
    got = forms[2].run(0, rays)
    mesh = got["kind"] == 2
    assert mesh.sum() >= 1575
    # f64 Moeller-Trumbore over all triangles (tests/trace_reference.py)
    t, _, _, _ = triangle_search(verts, tris, rays[mesh])
    order = np.argsort(t, axis=1)
    rows = np.arange(len(t))
    t0, t1 = t[rows, order[:, 0]], t[rows, order[:, 1]]
    assert np.isfinite(t0).all() and np.all(np.abs(t0 - got["t"][mesh]) <= 1e-4 * t0)
    tie = (t1 - t0) <= 1e-4 * t0  # a second triangle within 1e-4 t: the f32 walk may name either
    wrong = got["primitive"][mesh] != order[:, 0]
    print(f"primitive: {int(mesh.sum())} mesh hits, {int(tie.sum())} ties in f64, {int(wrong.sum())} differ from the f64 nearest")
    assert tie.sum() <= 0.01 * mesh.sum()
    assert not (wrong & ~tie).any()
    second = got["primitive"][mesh][wrong]
    assert np.all(second == order[wrong, 1]), "on a tie the other triangle of the pair"
    # terrain: the cell holds the hit position
    ter = got["kind"] == 1
    assert ter.sum() > 1500
    spacing = scenes.SPAN / (dem.shape[1] - 1)
    cx, cz = (got["primitive"][ter] & 0xFFFF).astype(np.float64), (got["primitive"][ter] >> 16).astype(np.float64)
    fx = (got["position"][ter, 0].astype(np.float64) - float(forms[2].origin[0])) / spacing
    fz = (got["position"][ter, 2].astype(np.float64) - float(forms[2].origin[1])) / spacing
    eps = 1e-4  # (f32 position at |x| <= 50 over a 1.6-unit cell: 4e-6 / 1.6 of a cell, with room)
    assert np.all((fx >= cx - eps) & (fx <= cx + 1 + eps) & (fz >= cz - eps) & (fz <= cz + 1 + eps))
    assert cx.max() < dem.shape[1] - 1 and cz.max() < dem.shape[0] - 1


# ---- bad rays --------------------------------------------------------------------------------------------------------------
def bad_ray_set(good):
    """`good` (n, 8) with bad rays mixed in: NaN and +-inf in every slot, a zero direction, a direction whose squared length
    leaves the f32 range, tmax == tmin and tmax < tmin.  Returns (rays, is_bad)."""
    bad = []
    base = good[: 8 * 3 + 5].copy()
    k = 0
    for slot in range(8):
        for value in (np.nan, np.inf, -np.inf):
            r = base[k].copy()
            r[slot] = value
            bad.append(r)
            k += 1
    for change in ("zero", "tiny", "huge", "equal", "reversed"):
        r = base[k].copy()
        if change == "zero":
            r[4:7] = 0.0
        elif change == "tiny":
            r[4:7] = np.float32(1e-30)
        elif change == "huge":
            r[4:7] = np.float32(3e30)
        elif change == "equal":
            r[7] = r[3]
        else:
            r[3], r[7] = 5.0, 1.0
        bad.append(r)
        k += 1
    bad = np.asarray(bad, np.float32)
    n = len(good) + len(bad)
    is_bad = np.zeros(n, bool)
    is_bad[np.linspace(1, n - 2, len(bad)).astype(int)] = True  # spread over the waves, never a whole wave
    rays = np.zeros((n, 8), np.float32)
    rays[is_bad], rays[~is_bad] = bad, good
    return rays, is_bad


def test_bad_rays_answer_as_a_miss_and_are_never_marched(city):
    forms, _, _, _, _, _, picked = city
    good = _rays_of(picked)[::16]  # 384 camera rays: sky, terrain and mesh
    rays, is_bad = bad_ray_set(good)
    assert is_bad.sum() == 29 and (is_bad.reshape(-1, 1)[: len(rays) // 64 * 64].reshape(-1, 64).sum(1) > 0).all(), "every wave holds bad rays among good ones"
    alone = forms[2].run(0, good)
    mixed = forms[2].run(0, rays)
    assert _same(alone, {k: v[~is_bad] for k, v in mixed.items()}), "the good rays answer as they do without the bad ones"
    assert (alone["kind"] == 0).any() and (alone["kind"] == 1).any() and (alone["kind"] == 2).any()
    assert not mixed["kind"][is_bad].any() and np.all(_bits(mixed["t"])[is_bad] == QNAN) and np.all(mixed["primitive"][is_bad] == NONE)
    assert not mixed["normal"][is_bad].any() and not mixed["position"][is_bad].any()
    assert not mixed["marches"][is_bad].any() and (mixed["marches"][~is_bad] == 1).all(), "one march per good ray, none for a bad one"
    for flags in (0, 2):
        occ_alone, occ = forms[2].run(1, good, flags=flags), forms[2].run(1, rays, flags=flags)
        assert np.array_equal(occ_alone["kind"], occ["kind"][~is_bad]) and not occ["kind"][is_bad].any()
        assert not occ["marches"][is_bad].any() and (occ["marches"][~is_bad] >= 1).all()


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_header_binding_and_layout():
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert "#define F3D_ABI_VERSION 6u" in header, "the query is additive: no ABI version bump"
    body = re.search(r"typedef struct f3d_session_query_desc \{(.*?)\} f3d_session_query_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    assert members == [name for name, _ in _native.QueryDesc._fields_]
    assert members == ["struct_size", "mode", "flags", "count", "rays", "kind", "t", "normal", "position", "primitive", "direction"]
    assert C.sizeof(_native.QueryDesc) == 16 + 7 * 8
    assert re.search(r"int f3d_session_query\(f3d_session \*session, const f3d_session_query_desc \*desc, char \*err, size_t errlen\);", header)
    entry = [e for e in _native.ABI if e[0] == "f3d_session_query"]
    assert len(entry) == 1 and entry[0][1] is C.c_int
    for name, value in (("CLOSEST", 0), ("OCCLUSION", 1), ("PIXELS", 2), ("TERRAIN_ONLY", 1), ("CURVED", 2), ("DEVICE_POINTERS", 4),
                        ("NO_WAIT", 8), ("SCRATCH_BYTES_PER_RAY", 80)):
        assert re.search(rf"#define F3D_QUERY_{name} {value}u", header) and getattr(_native, f"QUERY_{name}") == value


def test_wrapper_has_the_query_methods():
    from forge3d_amd.session import TerrainSession
    from forge3d_amd.viewer import ViewerHandle

    for name in ("trace", "occluded", "pick", "ground"):
        assert callable(getattr(TerrainSession, name))
    assert "7.2e-6" in TerrainSession.ground.__doc__ and "oracle" in TerrainSession.ground.__doc__
    assert "pick_at" in vars(ViewerHandle) and "NOT pinned" in ViewerHandle.pick_at.__doc__
