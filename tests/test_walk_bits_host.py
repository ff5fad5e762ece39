"""The raster lane bodies return the bits they returned at the commit tests/golden/raster_walk_bits.npz was made from.

The horizon, clearance and umbra walks (csrc/f3d_walk.h under f3d_horizon.h, f3d_clearance.h, f3d_umbra.h) and the lattice
point all five raster families stand their samples on, compiled for the host (the tests/*_host harnesses of THIS tree) and run
over the fixture's stored inputs: one-cell and one-cell-wide DEMs, the suites' ragged shapes, both wave footprints, flat and
curved, flat axes, lattice corners, observers on, beside and outside the lattice, straight-up directions, an injected step
cap.  Every plane's SHA-256 must equal the stored one.  The float64 references are the family suites' business
(tests/test_session_{horizon,clearance,umbra}_host.py); they allow a rounding to move, this does not.
The fixture's generator: tests/golden/make_walk_bits.py.
"""
from __future__ import annotations

from pathlib import Path

import pytest

import walk_bits as wb

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "raster_walk_bits.npz"


@pytest.fixture(scope="module")
def fixture():
    return wb.Fixture(FIXTURE)


@pytest.fixture(scope="module")
def harnesses():
    return wb.build_harnesses(ROOT)


def test_the_fixture_is_whole(fixture):
    assert len(fixture.want) == len(fixture.inputs["keys"]) and len(fixture.commit) == 40
    assert FIXTURE.stat().st_size < 262_272 // 2, "well under the largest committed fixture"
    for shape in wb.SHAPES:
        for family in ("horizon", "clearance", "umbra", "raster", "irradiation"):
            assert any(k.startswith(f"{family}/{wb.shape_name(shape)}/") for k in fixture.want)
    small = {wb.shape_name(s) for s in wb.SHAPES if s[0] * s[1] <= wb.FULL_PLANES_UP_TO}
    assert set(fixture.planes) == {k for k in fixture.want if k.split("/")[1] in small}
    for key, plane in fixture.planes.items():  # the planes held in full are the planes the digests are of
        assert wb.digest(plane) == fixture.want[key]


@pytest.mark.parametrize("shape", wb.SHAPES, ids=wb.shape_name)
def test_host_bodies_return_the_stored_bits(fixture, harnesses, shape):
    seen = set()
    for key, plane in wb.host_cases(harnesses, fixture.inputs, shape):
        seen.add(wb.stored_key(key))
        wrong = fixture.mismatch(key, plane)
        assert wrong is None, wrong
    assert seen == {k for k in fixture.want if k.split("/")[1] == wb.shape_name(shape)}, "every stored case was run"
