"""f3d_session_row_costs on the device: what the strip cutter of a multi-GPU job reads (forge3d_amd/distributed.py) -- the
frame kernel's per-tile wave times, spread over the image rows of the strip (csrc/f3d_tiles.h spread_tile_costs; the
arithmetic itself is checked on the host, tests/test_tiles_host.py)."""
from __future__ import annotations

import re

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

NO_COSTS_YET = ("no frame has left its tile costs yet (a one-band session with the default tile map does, from its first "
                "fused frame on)")


@pytest.mark.parametrize("rows", [None, (16, 50)], ids=["whole image", "rows 16-50"])
@pytest.mark.parametrize("variant", [0, 4000000, 8000000])
def test_row_costs_of_a_one_band_session(variant, rows):
    """112 x 80 on the golden DEM, one band, no frames in flight, default tile map, spp 8, with the automatic, the 4- and the
    8-lane frame kernel; the whole image and a strip whose 34 rows end in a ragged tile row of the 4-lane tile.  Before any
    frame there is nothing to report; after two frames every row has a finite, non-negative cost and the frame cost something."""
    from forge3d_amd.session import TerrainSession

    dem = scenes.golden_dem()
    kw = scenes.fixed_frames(scenes.scene_kwargs(dem), 2, spp=8)
    strip = {} if rows is None else dict(row_begin=rows[0], row_end=rows[1])
    want_rows = 80 if rows is None else rows[1] - rows[0]
    with TerrainSession(dem, 112, 80, scenes.CAM, kernel_variant=variant, frames_in_flight=0, bands=1, **strip, **kw) as s:
        with pytest.raises(ValueError, match=re.escape(NO_COSTS_YET)):
            s.row_costs()
        s.enqueue_frames(0, 2)
        cost = s.row_costs()
    assert cost.dtype == np.float32 and cost.shape == (want_rows,), (cost.dtype, cost.shape)
    assert np.all(np.isfinite(cost)) and np.all(cost >= 0.0), cost
    assert float(cost.astype(np.float64).sum()) > 0.0, cost
