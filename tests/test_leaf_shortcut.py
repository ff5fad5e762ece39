"""The leaf shortcut (csrc/f3d_trace.h leaf_shortcut): leaf solves whose outcome -- a clear miss, or for verdict-only callers
a clear crossing -- is read off the quadratic's coefficients instead of being found by the reference's root finder.  The
prediction has to be EXACT: tests/leaf_host/leaf_harness.cpp solves every leaf both ways and ends with a non-zero status on
the first disagreement (verdict, or a bit of t_hit); the emulator's renders with and without F3D_EMUL_NO_LEAF_SHORTCUT (host
builds only) are the same arrays; and on the headline frame the shortcut settles what it was built for."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import scenes
from emul import emul
from leaf_scenes import checker_scene, far_scene

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "leaf_host" / "leaf_harness.cpp"
KEYS = ("rgba", "albedo", "normal", "depth", "accum", "m2", "res")


@functools.lru_cache(maxsize=None)
def _program() -> Path:
    """The harness as a stand-alone program (its own main), with the emulator's flags."""
    out = Path(tempfile.mkdtemp(prefix="f3d_leaf_host_")) / "leaf_harness"
    flags = [f for f in emul.CXX if f not in ("-shared", "-fPIC")]
    subprocess.run([*flags, str(HARNESS), "-o", str(out)], check=True, capture_output=True)
    return out


def _run(*args):
    done = subprocess.run([str(_program()), *args], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout


def test_synthetic_leaves_on_and_around_every_threshold_solve_the_same_both_ways():
    """Set (i): 2 * 10^8 synthetic (dv0, dv1, dv2, t0, t1) over scales 1e-8 ... 1e5 -- random, nearly straight, 4 000 m heights
    with millimetre clearances, exact small integers (a = 0, b = 4 |a|, t0 == t1), grazing -- every leaf walked to each
    threshold of leaf_shortcut and solved on both sides of it to the ulp, +-0, denormals, the caps, NaN and +-inf in every slot."""
    out = _run("synthetic", "200")
    checked = int(re.search(r"synthetic: (\d+) leaf solves checked", out).group(1))
    assert checked >= 200_000_000, out


def test_every_leaf_the_marches_queue_on_the_golden_dem_solves_the_same_both_ways():
    """Set (ii): 10^5 random and lattice-aligned rays on tests/golden/mini_dem.npy at exaggerations 1, 20 and 37, with and
    without curvature, through the sorted descent, the march one lane at a time and the march in whole waves with the ray
    sharing live: every leaf they hand to the leaf solve is solved both ways.  All four outcomes occur among them."""
    out = _run("march", str(scenes.GOLDEN_DIR / "mini_dem.npy"))
    assert int(re.search(r"march: (\d+) rays", out).group(1)) >= 100_000, out
    for kind in ("closest-hit", "any-hit"):
        counts = [int(x) for x in re.search(kind + r" leaves: full (\d+), miss A (\d+), miss B (\d+), crossing (\d+)", out).groups()]
        assert min(counts) > 1000, (kind, counts)


def _render(dem, size, cam, shortcut, **kw):
    if not shortcut:
        os.environ["F3D_EMUL_NO_LEAF_SHORTCUT"] = "1"
    try:
        return emul.render(dem, size[0], size[1], cam, **kw)
    finally:
        os.environ.pop("F3D_EMUL_NO_LEAF_SHORTCUT", None)


RENDERS = {"checkerboard x 37, sun at 5 degrees": (checker_scene, dict(sample_lanes=4)),
           "1 000 m spacing, curvature on": (far_scene, dict(sample_lanes=8, frames_in_flight=2))}


@pytest.mark.parametrize("name", list(RENDERS))
def test_renders_are_the_same_arrays_with_and_without_the_shortcut(name):
    """Two small emulator scenes: every output array and the reservoirs, shortcut on against shortcut off -- and the
    oracle's image, so that the scenes are known to be renderable where the device tests use them."""
    from oracle import oracle

    scene, how = RENDERS[name]
    dem, cam, kw = scene()
    kw = scenes.fixed_frames(kw, 3, spp=4)
    on, off = (_render(dem, (64, 48), cam, shortcut, **kw, **how) for shortcut in (True, False))
    assert on["frames"] == off["frames"] and np.float32(on["variance"]) == np.float32(off["variance"]), name
    for key in KEYS:
        assert np.array_equal(on[key], off[key], equal_nan=True), (name, key)
    want = oracle.render(dem, 64, 48, cam, **kw)
    for key in ("rgba", "albedo", "normal", "depth"):
        assert np.array_equal(on[key], want[key], equal_nan=True), (name, key)
    assert np.isfinite(want["depth"]).mean() > 0.3, name  # (terrain fills a good part of the image)


@functools.lru_cache(maxsize=None)
def _tapped_library():
    """The harness once more, as a library: the emulator's entry points with the leaf tap behind them."""
    lib = emul.build_harness(HARNESS, "leaf_host")
    lib.emul_render.restype = C.c_int
    lib.emul_take_retraces.restype = C.c_uint64
    lib.emul_take_retraced.restype = C.c_uint64
    return lib


def test_on_the_headline_frame_at_most_a_tenth_of_the_any_hit_leaf_solves_take_the_full_path(monkeypatch):
    """Rows 480-512 of the headline frame (the rows profiles/README.md uses), every leaf tapped: the three tests settle at
    least 90 % of the leaf solves of the any-hit rays (sun and IBL occlusion) -- what the change is for -- and no tapped
    leaf solves differently with the shortcut."""
    from forge3d_amd import datasets

    lib = _tapped_library()
    monkeypatch.setattr(emul, "_lib", lib)
    dem, cam, kw = datasets.rainier_proxy_scene(2048)
    lib.leaf_tap_enable(C.c_int32(1))
    try:
        emul.render(dem, 1920, 1080, cam, rows=(480, 512), **dict(kw, spp=8, max_frames=2, min_frames=2, variance_threshold=1e30))
    finally:
        counts = (C.c_ulonglong * 9)()
        lib.leaf_tap_counts(counts)
        lib.leaf_tap_enable(C.c_int32(0))
    closest, any_hit, bad = list(counts[0:4]), list(counts[4:8]), counts[8]
    print("closest-hit leaves (full, A, B, crossing):", closest, " any-hit:", any_hit)
    assert bad == 0
    assert sum(any_hit) > 1_000_000, any_hit
    assert any_hit[0] <= 0.10 * sum(any_hit), any_hit
