"""The raster walks on the device return the bits tests/golden/raster_walk_bits.npz holds (tests/test_walk_bits_host.py: the
same fixture against the host build).

The fixture's stored inputs through f3d_session_horizon / _clearance / _umbra on sessions over its six DEMs -- among them the
one-cell DEM (2x2: one level, top == 0) and the one-cell-wide strips (2x9, 9x2: an axis collapses, every node of it ragged),
which the families' own device-against-host tests (from 5x3 up) do not reach.  Every plane's SHA-256 must equal the stored
one.  The injected-cap cases are left to the host test: the library has no such switch.
"""
from __future__ import annotations

from pathlib import Path

import pytest

import scenes
import walk_bits as wb
from test_gpu_reaim import H, W
from test_session_raster_host import _kw, shaped_dem

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "raster_walk_bits.npz"


@pytest.fixture(scope="module")
def fixture():
    return wb.Fixture(FIXTURE)


@pytest.mark.parametrize("shape", wb.SHAPES, ids=wb.shape_name)
def test_device_returns_the_stored_bits(fixture, shape):
    from forge3d_amd.session import TerrainSession

    dem = shaped_dem(shape)
    seen = set()
    with TerrainSession(dem, W, H, dict(scenes.CAM), **_kw(dem)) as s:
        for key, plane in wb.device_cases(s, fixture.inputs, shape):
            seen.add(key)
            wrong = fixture.mismatch(key, plane)
            assert wrong is None, wrong
    walked = {k for k in fixture.want if k.split("/")[1] == wb.shape_name(shape) and k.split("/")[0] in ("horizon", "clearance", "umbra")}
    assert seen == {k for k in walked if k.split("/")[4] != "cap" and k.split("/")[5] != "origins"}, "every stored case the library can express"
