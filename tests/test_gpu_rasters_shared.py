"""What the four raster families (f3d_session_raster / _horizon / _irradiation / _clearance) and the ray query share on the
host, on the device: csrc/f3d_host_rasters.h, f3d_host_query.h.

* the ORDER in which refusals win: raw descriptors that carry two faults at once, and the text that is raised.  The pairs
  follow the order of the checks family by family; results, regions, scratch sizes and every single refusal are pinned by
  tests/test_gpu_raster.py, _horizon.py, _irradiation.py, _clearance.py and _query.py;
* ONE scratch for the four families, at the sizes where the rounding of the layouts shows: a 1 x 1 region with one
  direction / azimuth / observer / term, the four host forms one after the other and then in reverse.
"""
from __future__ import annotations

import numpy as np
import pytest

import scenes
from test_gpu_clearance import _raw as raw_clearance
from test_gpu_horizon import _raw as raw_horizon
from test_gpu_irradiation import _raw as raw_irradiation
from test_gpu_query import _raw as raw_query
from test_gpu_raster import _city, _session
from test_gpu_raster import _raw as raw_raster
from test_session_horizon_host import compass
from test_session_irradiation_host import directions
from test_session_raster_host import sun_targets

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN, INF = float("nan"), float("inf")
NO_WAIT, SESSION_SUN = 8, 16
OUTSIDE, EMPTY = (64, 0, 1, 1), (0, 0, 0, 64)


@pytest.fixture(scope="module")
def city():
    """The 64x64 session of the families' refusal tests."""
    dem, _, _, kw = _city()
    with _session(dem, scenes.fixed_frames(kw, 4)) as s:
        yield s


T = np.ascontiguousarray(sun_targets())
AZ = np.ascontiguousarray(compass(16))
AZ_BAD = np.array([[0.0, -1.0], [NAN, 1.0]], f32)
TERMS = np.ascontiguousarray(directions())
OB = np.array([[3.0, 22.0, -4.0, 0.0], [-11.0, 19.0, 7.0, 0.0]], f32)
OB_BAD = np.array([[3.0, 22.0, -4.0, 0.0], [0.0, NAN, 0.0, 0.0]], f32)
RAYS = np.array([[0.0, 50.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1e30]], f32)


def _terms(*weights_or_rows):
    t = TERMS[:len(weights_or_rows)].copy()
    for row, change in zip(t, weights_or_rows):
        for slot, value in change.items():
            row[slot] = value
    return t


# "A > B": the descriptor carries A's fault and B's, and A's text is raised.
ORDER = [
    # raster: struct size, mode, flags, reserved, NO_WAIT, SESSION_SUN x 2, region x 2, lift, outputs, targets
    ("raster: bad mode > unknown flags", "raster mode must be", lambda s: raw_raster(s, T, mode=2, flags=32)),
    ("raster: unknown flags > reserved", "unknown raster flags", lambda s: raw_raster(s, T, flags=32, reserved=1)),
    ("raster: reserved > NO_WAIT without DEVICE_POINTERS", "reserved member must be 0", lambda s: raw_raster(s, T, flags=NO_WAIT, reserved=1)),
    ("raster: NO_WAIT > SESSION_SUN with targets", "NO_WAIT needs DEVICE_POINTERS", lambda s: raw_raster(s, T, flags=NO_WAIT | SESSION_SUN)),
    ("raster: SESSION_SUN with mode 0 > empty region", "SESSION_SUN is a direction", lambda s: raw_raster(s, None, mode=0, flags=SESSION_SUN, region=EMPTY)),
    ("raster: empty region > region outside", "empty raster region", lambda s: raw_raster(s, T, region=(64, 0, 0, 1))),
    ("raster: region outside > non-finite lift", "outside the 64x64 DEM", lambda s: raw_raster(s, T, region=OUTSIDE, lift=NAN)),
    ("raster: non-finite lift > both outputs null", "raster lift must be finite", lambda s: raw_raster(s, T, lift=INF, masks=False)),
    # horizon: struct size, flags, reserved, NO_WAIT, region x 2, lift, count, azimuths, outputs, the scan
    ("horizon: region outside > negative lift", "outside the 64x64 DEM", lambda s: raw_horizon(s, AZ, region=OUTSIDE, lift=-1.0)),
    ("horizon: negative lift > azimuth count 0", "horizon lift must be finite and not negative", lambda s: raw_horizon(s, AZ[:0], lift=-1.0)),
    ("horizon: null azimuths > both outputs null", "null azimuths", lambda s: raw_horizon(s, None, k=2, horizon=False)),
    ("horizon: both outputs null > non-finite azimuth", "both null", lambda s: raw_horizon(s, AZ_BAD, horizon=False)),
    # irradiation: struct size, flags, reserved, NO_WAIT, region x 2, lift, outputs, energy without directions, directions, the scan
    ("irradiation: non-finite lift > all outputs null", "irradiation lift must be finite", lambda s: raw_irradiation(s, TERMS, lift=NAN, energy=False)),
    ("irradiation: all outputs null > null directions", "all null", lambda s: raw_irradiation(s, None, k=2, energy=False)),
    # ("null directions > negative weight" cannot be sent: a weight is read through the pointer that is null.  What the order
    # of the checks says about the scan, the last check, is these two.)
    ("irradiation: all outputs null > negative weight", "all null", lambda s: raw_irradiation(s, _terms({3: -1.0}), energy=False)),
    ("irradiation: non-finite component > negative weight of the same direction", "direction 1 has a non-finite component",
     lambda s: raw_irradiation(s, _terms({}, {0: NAN, 3: -1.0}))),
    # clearance: struct size, flags, reserved, NO_WAIT, region x 2, count, observers, outputs, the scan
    ("clearance: region outside > observer count 0", "outside the 64x64 DEM", lambda s: raw_clearance(s, OB[:0], region=OUTSIDE)),
    ("clearance: null observers > both outputs null", "null observers", lambda s: raw_clearance(s, None, k=2, height=False)),
    ("clearance: both outputs null > non-finite observer", "both null", lambda s: raw_clearance(s, OB_BAD, height=False)),
    # query: struct size, mode, flags, NO_WAIT, CURVED outside mode 1, ...
    ("query: bad mode > unknown flags", "query mode must be", lambda s: raw_query(s, RAYS, mode=3, flags=16)),
    ("query: unknown flags > NO_WAIT without DEVICE_POINTERS", "unknown query flags", lambda s: raw_query(s, RAYS, flags=16 | NO_WAIT)),
    ("query: NO_WAIT > CURVED outside mode 1", "NO_WAIT needs DEVICE_POINTERS", lambda s: raw_query(s, RAYS, flags=NO_WAIT | 2)),
]


@pytest.mark.parametrize("text,call", [(t, c) for _, t, c in ORDER], ids=[name for name, _, _ in ORDER])
def test_of_two_faults_the_earlier_check_wins(city, text, call):
    before = city.info()["gpu_resource_bytes"]
    with pytest.raises(ValueError, match=text):
        call(city)
    assert city.info()["gpu_resource_bytes"] == before


# ---- one scratch for four families ---------------------------------------------------------------------------------------------
def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_one_scratch_for_four_families_at_the_sizes_where_the_rounding_shows():
    """One sample, one direction / azimuth / observer / term.  The four layouts (the outputs, rounded up to 16, then the
    input; the raster's count behind its targets), bytes:
        horizon, sky_view too       plane 4 + sky_view 4 -> 16, azimuth 8                   24
        clearance, lowest too       plane 4 + lowest 4 -> 16, observer 16                   32
        visibility, count too       mask word 8 -> 16, target 16, count 4                   36
        irradiation, all three      energy 4 + count 4 + normal 12 -> 32, direction 16      48
    The ledger counts what is asked for, to the byte: these are the figures info() reports."""
    dem, _, _, kw = _city()
    region, at = (5, 7, 1, 1), (5, 7)
    d, ob, term = T[:1, :3].copy(), OB[:1].copy(), TERMS[:1].copy()
    with _session(dem, kw) as s:
        whole = {"horizon": s.horizon(1, sky_view=True), "clearance": s.clearance(ob, lowest=True),
                 "visibility": s.visibility(d, toward=False, count=True), "irradiation": raw_irradiation(s, term, count=True, normal=True)}
    e, c, v = whole["irradiation"]
    whole["irradiation"] = (e.reshape(64, 64), c.reshape(64, 64), v.reshape(64, 64, 3))
    assert (whole["visibility"][1] <= 1).all() and np.isfinite(whole["horizon"][0]).any() and (np.abs(whole["irradiation"][2]).sum(-1) > 0).all()

    def window(name, got):
        for g, w in zip(got, whole[name]):
            assert _bits(np.asarray(g).reshape(-1), np.asarray(w[..., at[0], at[1]] if name != "irradiation" else w[at]).reshape(-1)), name

    calls = [("horizon", 24, lambda s: s.horizon(1, sky_view=True, region=region)),
             ("clearance", 32, lambda s: s.clearance(ob, lowest=True, region=region)),
             ("visibility", 36, lambda s: s.visibility(d, toward=False, count=True, region=region)),
             ("irradiation", 48, lambda s: raw_irradiation(s, term, count=True, normal=True, region=region))]
    with _session(dem, kw) as s:
        bytes0 = s.info()["gpu_resource_bytes"]
        for name, scratch, call in calls:
            window(name, call(s))
            assert s.info()["gpu_resource_bytes"] - bytes0 == scratch, f"after the {name} call"
        for name, _, call in reversed(calls):
            window(name, call(s))
            assert s.info()["gpu_resource_bytes"] - bytes0 == 48, f"a smaller call reuses the scratch ({name})"
