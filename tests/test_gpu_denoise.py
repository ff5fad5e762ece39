"""A-trous denoiser on the device: `forge3d_amd.denoise.atrous_denoise` over the cases and gates of tests/denoise_reference.py
(the ones tests/test_denoise_host.py puts the header's host build through): the non-finite pixels are the float64
reference's -- and the reference's own vector's, where forge3d's implementation answers --, the finite ones within the set's
tolerance, four times the float32 oracle's measured distance from float64.  Each case prints its largest error next to its
tolerance.  Then 40 passes, two calls back to back with different shapes, and the wrapper's conversions: float64, Fortran
order and strided input.  Nothing is larger than 40 x 52.
"""
from __future__ import annotations

import numpy as np
import pytest

import denoise_reference as dr

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = dr.cases()
BY_NAME = {c["name"]: c for c in CASES}


def _run(case):
    from forge3d_amd.denoise import atrous_denoise

    color, kw = dr.inputs(case)
    return atrous_denoise(color, **kw)


_WORST = {}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_against_float64(case, capsys):
    got = _run(case)
    ref = dr.want(case)
    ok = np.isfinite(ref) & np.isfinite(got)
    err = float(np.abs(got.astype(np.float64) - ref)[ok].max()) if ok.any() else 0.0
    with capsys.disabled():  # the figure first, then the gate
        print(f"denoise-gpu {case['name']}: {err:.3g} (tol {dr.TOL[case['set']]:.3g})")
    _WORST[case["set"]] = max(_WORST.get(case["set"], 0.0), err)
    dr.gate(case, got, dr.golden(case))


def test_device_errors_per_set(capsys):
    """(after the cases above) the largest device error of every parameter set, the figures DESIGN.md 9.2 quotes"""
    with capsys.disabled():
        for k, e in _WORST.items():
            print(f"denoise-gpu-set {k}: {e:.3g} (tol {dr.TOL[k]:.3g}, oracle {dr.MEASURED_ON_THE_ORACLE[k]:.3g})")
    assert all(e <= dr.TOL[k] for k, e in _WORST.items())


def test_a_nan_normal_is_not_swallowed():
    got = _run(BY_NAME["nan_normal_component_17x15_it2"])
    assert int(np.isnan(got).any(axis=-1).sum()) == 169  # as in the reference's own vector; a clamp that drops the NaN gives 0


def test_forty_passes():
    """Passes 29 and up run at the saturated spacing; from the sixth on every tap but the centre is outside the image."""
    for name in ("color_only_17x15_it40", "all_guides_17x15_it40"):
        err, tol = dr.gate(BY_NAME[name], _run(BY_NAME[name]))
        print(f"denoise-gpu {name}: {err:.3g} (tol {tol:.3g})")


def test_two_calls_back_to_back_with_different_shapes():
    """Nothing of a call outlives it: a small image after a large one and the other way round, each equal to its own run."""
    order = ("all_guides_3", "all_guides_3x5_it3", "all_guides_33x31_it3", "all_guides_1x1_it3", "all_guides_3")
    alone = {name: _run(BY_NAME[name]) for name in set(order)}
    for name in order:
        got = _run(BY_NAME[name])
        assert np.array_equal(got, alone[name], equal_nan=True), name
        dr.gate(BY_NAME[name], got, dr.golden(BY_NAME[name]))


def test_wrapper_converts_float64_fortran_and_strided_input():
    from forge3d_amd.denoise import atrous_denoise

    case = BY_NAME["all_guides_17x15_it2"]
    color, kw = dr.inputs(case)
    want = atrous_denoise(color, **kw)
    dr.gate(case, want, dr.golden(case))
    guides = ("albedo", "normal", "depth")

    def call(convert):
        return atrous_denoise(convert(color), **{**kw, **{g: convert(kw[g]) for g in guides}})

    def strided(a):  # every second row and third column of a larger array
        big = np.full((34, 45) + a.shape[2:], np.nan, a.dtype)
        big[::2, ::3] = a
        view = big[::2, ::3]
        assert not view.flags.c_contiguous
        return view

    for convert in (lambda a: a.astype(np.float64), np.asfortranarray, strided):
        got = call(convert)
        assert got.dtype == f32 and got.flags.c_contiguous and np.array_equal(got, want)
