"""Re-terrain of a live terrain session (f3d_session_reterrain: a re-aim under new DEM samples), the parts that need no GPU.

* The table passes' per-thread bodies (f3d_retable.h: what k_retable_tiles / k_retable_top run) on the host, in a shuffled
  thread order (tests/reterrain_host), over eleven DEM shapes -- 2x2 up to 512x512, axes that collapse early, widths one
  past a 64-cell tile -- and, per shape: the whole DEM, 1x1 blocks at every corner and inside, single rows and columns
  (the last ones included), a block across a tile border, 200 random blocks and chains of five blocks.  After every block
  the leaf table and every band level equal, byte for byte, the tables leaf_build_at / level_build_at / band_build_at
  build from scratch for the edited DEM (padding, +-inf records and -0.0 heights included), nothing outside the dirty
  range has been written (poisoned first), and level by level the min / max equal oracle.build_minmax_mips of the edited
  DEM x exaggeration.
* TerrainSession.reterrain and render_terrain_dem_sequence refuse what the wrapper refuses, with its types and texts,
  before the device is touched; the three older generators still refuse a per-frame heightmap.
* The header, the ctypes table and the descriptor's layout.
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import scenes
from emul import emul
from test_session_rearm_host import _no_device, _wrapper_error

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "reterrain_host" / "reterrain_harness.cpp"
SHAPES = ((2, 2), (3, 2), (2, 9), (17, 5), (33, 33), (64, 64), (65, 64), (100, 37), (129, 257), (257, 33), (512, 512))  # (w, h)
RANDOM_BLOCKS = 200
FIELDS = ("leaf", "band", "outside", "compared", "dirty_cells", "tiles")


@pytest.fixture(scope="module")
def harness():
    lib = emul.build_harness(HARNESS, "reterrain_host")
    lib.reterrain_chain.restype = C.c_int
    lib.reterrain_chain.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_uint64), C.c_void_p]
    lib.reterrain_stale.restype = C.c_int
    lib.reterrain_stale.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    return lib


def _dem(w, h, seed, special=True):
    """A w x h DEM with relief at every scale; `special`: some samples -0.0, +0.0 and exact ties."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-3.0, 9.0, (h, w)).astype(np.float32)
    if special:
        d[rng.random((h, w)) < 0.15] = np.float32(-0.0)
        d[rng.random((h, w)) < 0.15] = np.float32(0.0)
        d[rng.random((h, w)) < 0.05] = np.float32(2.5)
    return d


def _samples(rng, bw, bh, special=True):
    s = rng.uniform(-5.0, 12.0, (bh, bw)).astype(np.float32)
    if special:
        s[rng.random((bh, bw)) < 0.2] = np.float32(-0.0)
        s[rng.random((bh, bw)) < 0.1] = np.float32(0.0)
    return s


def _fixed_blocks(w, h):
    """(x0, y0, bw, bh): whole DEM, 1x1 at the corners and inside, single rows / columns with the last, across a tile border."""
    blocks = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1),
              (0, 0, w, 1), (0, h - 1, w, 1), (0, h // 2, w, 1), (0, 0, 1, h), (w - 1, 0, 1, h), (w // 2, 0, 1, h)]
    if w > 66:
        blocks += [(60, 0, 9, min(h, 3)), (63, h // 2, 3, 1), (64, 0, 1, h), (65, h - 1, 1, 1)]
    if h > 66:
        blocks += [(0, 60, min(w, 3), 9), (w // 2, 63, 1, 3), (0, 64, w, 1), (w - 1, 65, 1, 1)]
    if w > 130 and h > 130:
        blocks.append((50, 120, 100, 20))
    return blocks


def _random_block(rng, w, h):
    if rng.random() < 0.3:  # small edits are the common case
        bw, bh = int(rng.integers(1, min(w, 8) + 1)), int(rng.integers(1, min(h, 8) + 1))
    else:
        bw, bh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
    return int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1)), bw, bh


def _run(harness, dem, exaggeration, blocks, samples, exaggerations=None, seed=1, levels=False):
    """Apply the chain; returns (counts, edited DEM, levels or None)."""
    h, w = dem.shape
    d = np.ascontiguousarray(dem, np.float32).copy()
    rects = np.ascontiguousarray(blocks, np.uint32).reshape(-1, 4)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32).ravel() for s in samples]))
    ex = np.zeros(len(blocks), np.float32) if exaggerations is None else np.ascontiguousarray(exaggerations, np.float32)
    out = (C.c_uint64 * 6)()
    lv = None
    if levels:
        total, lw, lh = 0, 1 << max(w - 2, 0).bit_length(), 1 << max(h - 2, 0).bit_length()
        while True:
            total += lw * lh * 2
            if lw == 1 and lh == 1:
                break
            lw, lh = max(lw // 2, 1), max(lh // 2, 1)
        lv = np.zeros(total, np.float32)
    rc = harness.reterrain_chain(d.ctypes.data, w, h, exaggeration, len(blocks), rects.ctypes.data, flat.ctypes.data, ex.ctypes.data, seed, out,
                                 lv.ctypes.data if levels else None)
    assert rc == 0, f"chain refused ({rc})"
    return dict(zip(FIELDS, (int(x) for x in out))), d, lv


def _clean(r, what):
    assert r["compared"] > 0
    assert r["leaf"] == 0, f"{what}: {r['leaf']} leaf records differ from the build from scratch"
    assert r["band"] == 0, f"{what}: {r['band']} band records differ from the build from scratch"
    assert r["outside"] == 0, f"{what}: {r['outside']} records outside the dirty range were written"


def _against_oracle(lv, dem, exaggeration, what):
    from oracle import oracle

    want, dims = oracle.build_minmax_mips((dem * np.float32(exaggeration)).astype(np.float32))
    off = 0
    for l, ((pw, ph), level) in enumerate(zip(dims, want)):
        got = lv[off:off + pw * ph * 2].reshape(ph, pw, 2)
        assert np.array_equal(got, level), f"{what}: level {l} ({pw}x{ph}) differs from oracle.build_minmax_mips"
        off += pw * ph * 2
    assert off == lv.size, f"{what}: {lv.size} level values, the oracle's chain has {off}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_patched_tables_equal_the_build_from_scratch(harness, shape):
    w, h = shape
    rng = np.random.default_rng(1000 * w + h)
    exaggeration = float(np.float32(rng.uniform(0.3, 7.0)))
    dem = _dem(w, h, 7 * w + h)
    # every fixed block and every random one on its own, from the original DEM
    blocks = _fixed_blocks(w, h) + [_random_block(rng, w, h) for _ in range(RANDOM_BLOCKS)]
    dirty = tiles = 0
    for k, b in enumerate(blocks):
        s = _samples(rng, b[2], b[3])
        r, edited, lv = _run(harness, dem, exaggeration, [b], [s], seed=17 * k + 3, levels=k % 8 == 0 or k < 12)
        _clean(r, f"{w}x{h} block {b}")
        want = dem.copy()
        want[b[1]:b[1] + b[3], b[0]:b[0] + b[2]] = s
        assert np.array_equal(edited.view(np.uint32), want.view(np.uint32))
        if lv is not None:
            _against_oracle(lv, edited, exaggeration, f"{w}x{h} block {b}")
        dirty += r["dirty_cells"]
        tiles += r["tiles"]
    assert dirty >= len(blocks) and tiles >= len(blocks)
    # chains of five, each on the tables the one before left; every third chain ends with the whole DEM under another exaggeration
    for c in range(12):
        chain = [_random_block(rng, w, h) for _ in range(5)]
        ex = [0.0] * 5
        if c % 3 == 2:
            chain[4] = (0, 0, w, h)
            ex[4] = float(np.float32(rng.uniform(0.5, 3.0)))
        if c % 3 == 1:
            chain[0] = (0, 0, w, h)
        samples = [_samples(rng, b[2], b[3]) for b in chain]
        r, edited, lv = _run(harness, dem, exaggeration, chain, samples, ex, seed=900 + c, levels=True)
        _clean(r, f"{w}x{h} chain {chain}")
        _against_oracle(lv, edited, ex[4] or exaggeration, f"{w}x{h} chain {chain}")


def test_products_that_overflow_and_signed_zeros_keep_the_builders_bits(harness):
    """Finite heights whose product with the exaggeration is +-inf, and DEMs of nothing but signed zeros."""
    rng = np.random.default_rng(5)
    for w, h in ((9, 9), (65, 64), (130, 70)):
        dem = _dem(w, h, 11)
        dem[rng.random((h, w)) < 0.1] = np.float32(3.0e38)
        dem[rng.random((h, w)) < 0.1] = np.float32(-3.0e38)
        for k in range(40):
            b = _random_block(rng, w, h)
            s = _samples(rng, b[2], b[3])
            s[rng.random(s.shape) < 0.2] = np.float32(3.0e38)
            s[rng.random(s.shape) < 0.2] = np.float32(-3.0e38)
            r, _, _ = _run(harness, dem, 2.0, [b], [s], seed=k)
            _clean(r, f"{w}x{h} overflowing block {b}")
        zeros = np.where(rng.random((h, w)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        for k in range(40):
            b = _random_block(rng, w, h)
            s = np.where(rng.random((b[3], b[2])) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            r, _, _ = _run(harness, zeros, 1.5, [b], [s], seed=k)
            _clean(r, f"{w}x{h} signed-zero block {b}")


def test_the_harness_sees_levels_that_were_not_rebuilt(harness):
    """The comparison can fail: leaves and level 0 patched, the levels above left as they were."""
    dem = _dem(130, 70, 3, special=False)
    s = np.full((5, 5), 100.0, np.float32)
    rect = np.asarray([40, 30, 5, 5], np.uint32)
    out = (C.c_uint64 * 2)()
    d = dem.copy()
    assert harness.reterrain_stale(d.ctypes.data, 130, 70, 1.0, rect.ctypes.data, s.ctypes.data, out) == 0
    assert out[0] == 0 and out[1] >= 7, list(out)  # (every level above 0 holds the old maximum somewhere)


# ---- TerrainSession.reterrain and render_terrain_dem_sequence: what they refuse, before any device work ----------------------
CAM_B = {"origin": (40.0, 30.0, 80.0), "look_at": (0.0, 5.0, 0.0), "up": (0.0, 1.0, 0.0), "fov_y": 50.0}


def _bare_session(shape=(32, 32)):
    """A TerrainSession that has no library: whatever reaches the native call raises."""
    from forge3d_amd.session import TerrainSession

    s = TerrainSession.__new__(TerrainSession)
    s.dem_shape = shape
    s._camera = {}
    s._armed = {"sun_azimuth_deg": 315.0, "sun_elevation_deg": 45.0, "sun_intensity": 2.5, "sun_color": (1.0, 0.97, 0.92), "exposure": 1.0,
                "env_intensity": 0.35, "seed": 7, "max_frames": 8, "min_frames": 8, "variance_threshold": 1e-3, "observer_latitude_deg": 0.0,
                "observer_longitude_deg": 0.0, "pressure_mbar": 1013.25, "temperature_c": 15.0}

    class _Lib:
        def __getattr__(self, name):
            raise AssertionError("the device was touched")

    s._lib = _Lib()
    s._handle = None
    return s


def test_reterrain_checks_its_arguments_before_the_native_call():
    s = _bare_session()
    try:
        with pytest.raises(ValueError, match=re.escape("heightmap must be 2D (H, W), got shape (32,)")):
            s.reterrain(np.zeros(32, np.float32))
        with pytest.raises(ValueError, match=re.escape("heightmap has shape (16, 32), the session's DEM has (32, 32): a patch needs at=(row, col)")):
            s.reterrain(np.zeros((16, 32), np.float32))
        with pytest.raises(ValueError, match="must not be negative"):
            s.reterrain(np.zeros((4, 4), np.float32), at=(-1, 0))
        with pytest.raises(TypeError, match="reterrain\\(\\) got an unexpected keyword argument 'spp'"):
            s.reterrain(np.zeros((32, 32), np.float32), spp=4)
        with pytest.raises(OverflowError):
            s.reterrain(np.zeros((32, 32), np.float32), seed=-1)
        # what the wrapper accepts gets as far as the native layer
        with pytest.raises(AssertionError, match="the device was touched"):
            s.reterrain(np.zeros((32, 32), np.float32))
        with pytest.raises(AssertionError, match="the device was touched"):
            s.reterrain(np.zeros((3, 5), np.float32), CAM_B, at=(29, 27), seed=3)
    finally:
        s._handle = None


@pytest.mark.parametrize("key,value", [("spp", 4), ("width", 64), ("spacing", (2.0, 2.0)), ("env_map", None), ("atmosphere", None), ("exposure", 2.0),
                                       ("mesh_vertices", np.zeros((3, 3), np.float32))])
def test_dem_sequence_refuses_a_key_a_live_session_cannot_change(monkeypatch, key, value):
    from forge3d_amd.path_tracing import render_terrain_dem_sequence

    _no_device(monkeypatch)
    dem = scenes.golden_dem(8)
    frames = [{}, {"heightmap": dem + 1.0, "sun_azimuth_deg": 20.0, key: value}]
    with pytest.raises(ValueError, match=re.escape(f"frames[1] sets {key!r}")):
        list(render_terrain_dem_sequence(dem, 32, 24, scenes.CAM, frames=frames, **scenes.scene_kwargs(dem)))


def test_dem_sequence_refuses_another_dem_shape_naming_both(monkeypatch):
    from forge3d_amd.path_tracing import render_terrain_dem_sequence

    _no_device(monkeypatch)
    dem = scenes.golden_dem(8)
    kw = scenes.scene_kwargs(dem)
    other = np.zeros((dem.shape[0], dem.shape[1] + 1), np.float32)
    text = re.escape(f"frames[2] has a heightmap of shape {other.shape}, the sequence's DEM has {dem.shape}")
    with pytest.raises(ValueError, match=text):
        list(render_terrain_dem_sequence(dem, 32, 24, scenes.CAM, frames=[{}, {"heightmap": dem * 2.0}, {"heightmap": other}], **kw))
    with pytest.raises(TypeError, match="unexpected keyword argument 'bogus'"):
        list(render_terrain_dem_sequence(dem, 32, 24, scenes.CAM, frames=[{}], bogus=1, **kw))
    assert list(render_terrain_dem_sequence(dem, 32, 24, scenes.CAM, frames=[], **kw)) == []


def test_the_other_sequences_still_refuse_a_heightmap_per_frame(monkeypatch):
    from forge3d_amd.path_tracing import render_terrain_camera_sequence, render_terrain_mesh_sequence, render_terrain_sequence

    _no_device(monkeypatch)
    dem = scenes.golden_dem(8)
    v, t = scenes.box_city(n_boxes=6, seed=5, span=40.0)
    kw = scenes.scene_kwargs(dem)
    text = re.escape("frames[1] sets 'heightmap', which a live session cannot change")
    with pytest.raises(ValueError, match=text):
        list(render_terrain_sequence(dem, 32, 24, scenes.CAM, frames=[{}, {"heightmap": dem + 1.0}], **kw))
    with pytest.raises(ValueError, match=text):
        list(render_terrain_camera_sequence(dem, 32, 24, frames=[{"camera": scenes.CAM}, {"camera": CAM_B, "heightmap": dem + 1.0}], **kw))
    with pytest.raises(ValueError, match=text):
        list(render_terrain_mesh_sequence(dem, 32, 24, scenes.CAM, frames=[{}, {"heightmap": dem + 1.0}], mesh_vertices=v, mesh_indices=t, **kw))


def test_dem_sequence_refuses_what_the_wrapper_refuses_with_its_types_and_messages(monkeypatch):
    """Every frame goes through the wrapper's own checks -- with ITS DEM, exaggeration, camera and values -- before the device is touched."""
    from forge3d_amd import path_tracing
    from forge3d_amd.path_tracing import hybrid_render_terrain_reference, render_terrain_dem_sequence

    _no_device(monkeypatch)
    monkeypatch.setattr(path_tracing._NATIVE, "hybrid_render_terrain_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("rendered")))
    dem = scenes.golden_dem(8)
    kw = scenes.scene_kwargs(dem)
    kw.pop("sun_azimuth_deg"), kw.pop("sun_elevation_deg")
    when = {"datetime_utc": "2024-06-21T12:00:00Z", "latitude_deg": 46.85, "longitude_deg": -121.76}
    good = {"sun_azimuth_deg": 1.0}
    nan = dem.copy()
    nan[3, 4] = np.nan
    inf = dem.copy()
    inf[0, 0] = np.inf
    cases = [
        ({}, [good, {"heightmap": nan}]),                                               # non-finite samples in frame 1
        ({}, [good, {"heightmap": inf}]),
        ({}, [good, {"heightmap": np.zeros(16, np.float32)}]),                          # a DEM that is not 2-D
        ({}, [good, {"heightmap": np.zeros((1, 5), np.float32)}]),                      # smaller than 2x2
        ({}, [good, {"heightmap": dem, "camera": 5}]),                                  # a camera that is no mapping
        ({}, [{"heightmap": dem, "solar_time": when, "sun_azimuth_deg": 10.0}]),        # solar_time + manual angles
        ({}, [good, {"heightmap": dem, "sun_color": (1.0, -1.0, 0.5)}]),                # a bad colour in frame 1
        ({}, [good, {"heightmap": dem, "min_frames": 600, "max_frames": 512}]),         # budget order
        ({}, [good, {"exaggeration": "tall"}]),                                         # an exaggeration that is no number
        ({"spp": 65}, [good]),
    ]
    for common, frames in cases:
        for frame in frames:
            rest = {k: val for k, val in frame.items() if k not in ("camera", "heightmap")}
            want = _wrapper_error(lambda: hybrid_render_terrain_reference(frame.get("heightmap", dem), 32, 24, frame.get("camera", scenes.CAM),
                                                                          **{**kw, **common, **rest}))
            if want is not None:
                break
        assert want is not None, (common, frames)
        with pytest.raises(want[0]) as got:
            list(render_terrain_dem_sequence(dem, 32, 24, scenes.CAM, frames=frames, **kw, **common))
        assert str(got.value) == want[1]
    # frames the wrapper accepts get as far as the native layer
    with pytest.raises(AssertionError, match="the device was touched"):
        list(render_terrain_dem_sequence(dem, 32, 24, scenes.CAM, frames=[good, {"heightmap": dem * 0.5, "exaggeration": 3.0, "camera": CAM_B}], **kw))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_declare_the_reterrain_entry_point():
    from forge3d_amd import _native

    header = (ROOT / "include" / "f3d_terrain_pt.h").read_text()
    assert re.search(r"\bf3d_session_reterrain\s*\(", header)
    assert "f3d_session_reterrain" in {n for n, _, _ in _native.ABI}
    assert "#define F3D_ABI_VERSION 6u" in header and _native.ABI_VERSION == 6  # additive: detected by the symbol
    body = re.search(r"typedef struct f3d_session_reterrain_desc \{(.*?)\} f3d_session_reterrain_desc;", header, re.S).group(1)
    assert body.split(";")[0].split() == ["uint32_t", "struct_size"]
    fields = ("heights", "width", "height", "x0", "y0", "exaggeration", "aim")
    R = _native.ReterrainDesc
    assert [n for n, _ in R._fields_] == ["struct_size", *fields]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f3d_terrain_pt.h"\nint main(void) { printf("%zu %zu ' + \
          " ".join(["%zu"] * len(fields)) + '\\n", sizeof(f3d_session_reterrain_desc), sizeof(f3d_session_reaim_desc), ' + \
          ", ".join(f"offsetof(f3d_session_reterrain_desc, {f})" for f in fields) + "); return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "layout.c"
        c.write_text(src)
        exe = Path(tmp) / "layout"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(R), C.sizeof(_native.ReaimDesc), *(getattr(R, f).offset for f in fields)]
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.library_path())], capture_output=True, text=True, check=True)
    assert any(line.split()[-1] == "f3d_session_reterrain" and " T " in line for line in out.stdout.splitlines())
    text = (ROOT / "INTEGRATION.md").read_text()
    assert "pub struct F3dSessionReterrainDesc" in text and "f3d_session_reterrain" in text
    for comment in ("DEM and exaggeration (see f3d_session_reterrain), spacing, mesh (see f3d_session_remesh)",
                    "exaggeration (see f3d_session_reterrain), spacing, mesh (see f3d_session_remesh), environment map, image size, strip rows and spp stay"):
        assert comment in header
