"""The HIP smoke solver (SmokeDomain.step, csrc/f3d_smoke_sim.hip) against the float64 statement of a step
(tests/smoke_sim_reference.py): the sets of test_smoke_sim_reference_host.py part b, one step at a time from the device's own
float32 state of the step before, under the gates and band caps that were measured on the oracle.  No oracle, no emulator."""
from __future__ import annotations

import numpy as np
import pytest

import smoke_sim_cases as cases
import smoke_sim_reference as ref

pytestmark = pytest.mark.gpu


def _domain(name):
    from forge3d_amd import smoke

    geo, emitters, settings, steps, seeder = cases.reference_sets()[name]
    dom = smoke.SmokeDomain(geo["dims"], geo.get("voxel_size", (1.0, 1.0, 1.0)), geo.get("origin", (0.0, 0.0, 0.0)),
                            sparse_threshold=cases.REFERENCE_THRESHOLD)
    seeder(dom)
    return dom, emitters, settings, steps


def _hold_to_the_gate(name, dom, want, masks, step):
    assert dom.frame_index == want["frame_index"] and abs(dom.time_seconds - want["time_seconds"]) <= 4 * ref.EPS32 * want["time_seconds"]
    for field, (err, share) in ref.residuals({f: getattr(dom, f) for f in ref.FIELDS}, want, masks).items():
        print(f"smoke-ref-gpu {name:26s} step {step} {field:14s} {err:8.2f} eps32*max|ref|   left out {share:.5f}")
        assert share <= ref.BAND_CAP, (name, step, field, share)
        assert err <= ref.gate(name, field), (name, step, field, err, ref.gate(name, field))


@pytest.mark.parametrize("form", ["default", "launches"])
@pytest.mark.parametrize("name", sorted(cases.reference_sets()))
def test_hip_solver_equals_the_reference(name, form, monkeypatch):
    from forge3d_amd import smoke

    if form == "launches":
        monkeypatch.setenv("F3D_SMOKE_SOLVER", "launches")
    else:
        monkeypatch.delenv("F3D_SMOKE_SOLVER", raising=False)
    dom, emitters, settings, steps = _domain(name)
    s, em = ref.settings(**settings), [ref.emitter(**e) for e in emitters]
    device_emitters = [smoke.SmokeEmitter(**e) for e in emitters]
    for k in range(steps):
        want, masks = ref.step(ref.promote(dom, dims=dom.dims), s, em)
        dom.step(smoke.SmokeStepSettings(**settings), device_emitters, steps=1)
        _hold_to_the_gate(name, dom, want, masks, k)
    assert float(dom.density.max()) > 50 * cases.REFERENCE_THRESHOLD


def test_resident_state_equals_the_host_path_and_the_reference():
    """The nine fields device-resident (SmokeSequence steps them in place, nothing crosses the bus): after the same steps the
    state equals the host-array path's bit for bit, and every step passes the reference's gate."""
    from forge3d_amd import smoke

    name = "case-turbulent_wind"  # every sum, the lane shear, a non-cubic voxel, an emitter that starts and one that ends
    host, emitters, settings, steps = _domain(name)
    resident, _, _, _ = _domain(name)
    s, em = ref.settings(**settings), [ref.emitter(**e) for e in emitters]
    device_emitters = [smoke.SmokeEmitter(**e) for e in emitters]
    seq = smoke.SmokeSequence(resident, np.zeros((8, 8, 4), np.uint8), camera_pos=(0.0, 30.0, -40.0), target=(10.0, 5.0, 10.0))
    try:
        for k in range(steps):
            want, masks = ref.step(ref.promote(resident, dims=resident.dims), s, em)
            seq.step(smoke.SmokeStepSettings(**settings), device_emitters, steps=1)
            host.step(smoke.SmokeStepSettings(**settings), device_emitters, steps=1)
            seq.download()
            assert resident.frame_index == host.frame_index and np.float32(resident.time_seconds) == np.float32(host.time_seconds)
            for field in ref.FIELDS:
                assert np.array_equal(getattr(resident, field), getattr(host, field)), (k, field)
            _hold_to_the_gate(name, resident, want, masks, k)
    finally:
        seq.close()
