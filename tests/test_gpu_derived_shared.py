"""What the derived families (f3d_session_fill / _drainage / _streams / _contours) share on the host, on the device:
csrc/f3d_host_derived.h and the layouts of csrc/f3d_scratch_carve.h.

ONE scratch for them, the rasters' own: on the 65x63 x2.5 DEM -- partial tiles, more than one wave, a row length that is no
multiple of 64 -- the host forms one after the other on one session and then in reverse; every result has the bytes of the
same call on a fresh session -- where the tracked bytes rise by exactly the call's total --, and on the shared session the
tracked bytes are those of the largest call so far.  Results, regions and every refusal of a family are pinned by
tests/test_gpu_contour.py, _drainage.py and _fill.py; the layouts' arithmetic, piece by piece, by
tests/test_scratch_carve_host.py, whose formulas give the totals here.
"""
from __future__ import annotations

import numpy as np
import pytest

import drainage_cases as cases
from test_gpu_drainage import _session
from test_scratch_carve_host import A, drainage, drainage_pieces, fill, filled_drainage

pytestmark = pytest.mark.gpu

SAMPLES, TILES = 65 * 63, 2  # (the fill's tiles have an edge of 64: 2 x 1)
# The scratch of the two calls whose count layout holds rocPRIM's scan storage -- a figure only the device names -- is what a
# session of commit 2877084, BEFORE the layouts were carved, reported for each call on an MI355X (3 485 stream segments, 1 158
# contour segments; by the formulas both leave 1 280 bytes for the scan); every other figure follows from the formulas.
STREAMS_BYTES, CONTOURS_BYTES = 194560, 26624
SCHEDULE = ("fill_rounds", "flat_rounds")  # (the rounds of the tiled relaxations depend on the device's schedule)


def _bytes(result):
    return {k: (v.dtype.str, v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v for k, v in result.items() if k not in SCHEDULE}


def test_one_scratch_for_the_derived_families_forward_and_in_reverse():
    """The totals, bytes (n = 4095 samples, A rounds up to 256):
        fill(), the surface alone       A(4 * 1024) + 2 A(4 * 2) + 3 A(4n), then A(4n)
        filled.drainage(basin=True)     A(4 * 8960) + A(n) + 5 A(4n), the fill's pieces, then A(n) + 2 A(4n)
        drainage()                      the routing's pieces, then A(n) + A(4n)
        streams(2)                      the routing's pieces, the count layout, then the records: as observed
        contours(interval=0.25)         the count layout, then the records: as observed
        drainage() of one sample        the routing's pieces, then 256 + 256
    grow_scratch takes exactly what a call asks for when that is more than the scratch holds, and nothing otherwise: after
    each call the tracked bytes are the largest total so far, and the reversed pass, whose first call is no larger, adds none."""
    dem, spacing, e = cases.named_cases()["65x63 x2.5"]
    kw = cases.shape_kw(dem, spacing, e)
    assert dem.size == SAMPLES
    one = (40, 37, 1, 1)
    calls = [("fill", fill(SAMPLES, TILES, 1, 0)[1], lambda s: s.fill()),
             ("filled drainage", filled_drainage(SAMPLES, TILES, 7, 0)[1], lambda s: s.filled.drainage(basin=True)),
             ("drainage", drainage(SAMPLES, 3, 0)[1], lambda s: s.drainage()),
             ("streams", STREAMS_BYTES, lambda s: s.streams(2)),
             ("contours", CONTOURS_BYTES, lambda s: s.contours(interval=0.25)),
             ("drainage of one sample", drainage_pieces(SAMPLES)[1] + A(1) + A(4), lambda s: s.drainage(one))]
    fresh = {}
    for name, scratch, call in calls:
        with _session(dem, kw) as s:
            bytes0 = s.info()["gpu_resource_bytes"]
            fresh[name] = _bytes(call(s))
            print(f"{name} on a session of its own: scratch {s.info()['gpu_resource_bytes'] - bytes0}, expected {scratch}")
            assert s.info()["gpu_resource_bytes"] - bytes0 == scratch, f"the {name} call alone"
    assert fresh["streams"]["total"] > 64 and fresh["contours"]["total"] > 64 and fresh["fill"]["filled_samples"] > 0
    with _session(dem, kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        most = 0
        for name, scratch, call in calls:
            assert _bytes(call(s)) == fresh[name], name
            most = max(most, scratch)
            print(f"{name}: scratch {s.info()['gpu_resource_bytes'] - bytes0}, the largest total so far {most}")
            assert s.info()["gpu_resource_bytes"] - bytes0 == most, f"after the {name} call"
        for name, _, call in reversed(calls):
            assert _bytes(call(s)) == fresh[name], f"{name}, reversed"
            assert s.info()["gpu_resource_bytes"] - bytes0 == most, f"a smaller call reuses the scratch ({name})"
