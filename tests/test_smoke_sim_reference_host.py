"""The float64 statement of a smoke-solver step (tests/smoke_sim_reference.py), without a GPU:
  a. the statement against known answers, pass by pass;
  b. the oracle (oracle/smoke_sim_oracle.c) against the statement, one step at a time from the oracle's own float32 state of the
     step before -- this prints the table smoke_sim_reference.MEASURED_ON_THE_ORACLE records (-s | grep smoke-ref);
  c. the gate has teeth: three slightly wrong steppers fail it, by the field the change touches."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import smoke_sim_cases as cases
import smoke_sim_reference as ref
from oracle import smoke_oracle as so


# ---- a. known answers --------------------------------------------------------------------------------------------------------
def _grid(nx, ny, nz):
    return ref.lattice((nz, ny, nx))


def test_trilinear_is_exact_on_a_linear_field_and_clamps_outside():
    z, y, x = _grid(7, 5, 6)
    field = 0.25 * x - 1.5 * y + 3.0 * z + 2.0
    rng = np.random.default_rng(0)
    px, py, pz = rng.uniform(0, 6, 200), rng.uniform(0, 4, 200), rng.uniform(0, 5, 200)
    np.testing.assert_allclose(ref.trilinear(field, px, py, pz), 0.25 * px - 1.5 * py + 3.0 * pz + 2.0, rtol=0, atol=1e-13)
    vec = np.stack([field, 2.0 * field, -field], -1)
    np.testing.assert_allclose(ref.trilinear(vec, px, py, pz)[:, 1], 2.0 * (0.25 * px - 1.5 * py + 3.0 * pz + 2.0), rtol=0, atol=1e-13)
    # outside: the value of the nearest point of the grid
    assert ref.trilinear(field, np.array([-3.0]), np.array([2.0]), np.array([9.0]))[0] == field[5, 2, 0]
    assert ref.trilinear(field, np.array([40.0]), np.array([-1.0]), np.array([-0.5]))[0] == field[0, 0, 6]
    assert ref.trilinear(field, np.array([6.0]), np.array([4.0]), np.array([5.0]))[0] == field[5, 4, 6]  # the last lattice point itself


def test_divergence_of_a_linear_flow():
    z, y, x = _grid(6, 5, 7)
    a, b, c = 0.3, -0.2, 0.7
    hx, hy, hz = 1.5, 0.5, 2.0  # the flow is stated in world units: u = a * (x hx)
    v = np.stack([a * x * hx, b * y * hy, c * z * hz], -1)
    d = ref.divergence(v, (hx, hy, hz))
    inner = np.zeros(d.shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    np.testing.assert_allclose(d[inner], a + b + c, rtol=1e-13)
    assert (d[~inner] == 0.0).all()


def test_curl_of_a_rigid_rotation_is_twice_its_angular_velocity():
    z, y, x = _grid(6, 7, 5)
    h = (1.5, 1.0, 2.0)
    w = np.array([0.3, -0.5, 0.2])
    r = np.stack([x * h[0], y * h[1], z * h[2]], -1)
    c = ref.curl(np.cross(np.broadcast_to(w, r.shape), r), h)
    np.testing.assert_allclose(c[1:-1, 1:-1, 1:-1], np.broadcast_to(2.0 * w, c[1:-1, 1:-1, 1:-1].shape), rtol=0, atol=1e-13)
    assert (c[0] == 0.0).all() and (c[:, 0] == 0.0).all() and (c[:, :, -1] == 0.0).all()


def test_a_whole_voxel_flow_shifts_a_scalar_exactly():
    rng = np.random.default_rng(1)
    field = rng.random((6, 5, 9))
    h, dt = (1.5, 1.0, 2.0), 0.5
    v = np.zeros(field.shape + (3,))
    v[..., 0] = 2.0 * h[0] / dt  # two voxels a step towards +x
    out = ref.advect_scalar(field, v, h, dt, False)
    assert np.array_equal(out[:, :, 2:], field[:, :, :-2])  # away from the inflow face: the field, two voxels on
    assert np.array_equal(out[:, :, :2], np.repeat(field[:, :, :1], 2, axis=2))  # the inflow face's value fills what it uncovered
    back = ref.departure(v, h, dt)
    assert not ref.maccormack_band(back).any()  # on the lattice exactly: not in the band
    # The correction's round trip ends where it began, so it takes half of (field - predictor) here, and clamps that to the
    # eight cells whose lowest corner is the back-traced voxel -- written out voxel by voxel
    corrected = ref.advect_scalar(field, v, h, dt, True)
    nz, ny, nx = field.shape
    for z, y, x in [(0, 0, 0), (2, 3, 5), (5, 4, 8), (3, 0, 1), (4, 2, 2)]:
        x0 = max(x - 2, 0)
        cells = field[z:min(z + 2, nz), y:min(y + 2, ny), x0:min(x0 + 2, nx)]
        assert corrected[z, y, x] == min(max(out[z, y, x] + 0.5 * (field[z, y, x] - out[z, y, x]), cells.min()), cells.max())


def test_diffusion_keeps_a_constant_and_conserves_a_compact_interior_sum():
    const = np.full((6, 7, 8), 3.25)
    np.testing.assert_allclose(ref.diffuse(const, 0.3, 0.5), const, rtol=1e-15)
    blob = np.zeros((9, 9, 9))
    blob[3:6, 3:6, 3:6] = np.random.default_rng(2).random((3, 3, 3))
    out = ref.diffuse(blob, 0.3, 0.5)
    np.testing.assert_allclose(out.sum(), blob.sum(), rtol=1e-13)
    assert out[2, 4, 4] > 0.0 and out[1, 4, 4] == 0.0  # one ring a pass
    assert ref.diffuse(blob, 0.0, 0.5) is blob


def test_a_jacobi_sweep_returns_a_solution_of_the_discrete_poisson_equation():
    rng = np.random.default_rng(3)
    p = np.zeros((7, 6, 8))
    p[1:-1, 1:-1, 1:-1] = rng.normal(size=(5, 4, 6))
    ring = sum(np.roll(p, s, axis) for axis in range(3) for s in (-1, 1))
    div = np.zeros_like(p)
    div[1:-1, 1:-1, 1:-1] = (ring - 6.0 * p)[1:-1, 1:-1, 1:-1]  # so that p = (ring - div) / 6 in the interior
    np.testing.assert_allclose(ref.jacobi_sweep(p, div), p, rtol=0, atol=1e-14)


def test_two_hundred_sweeps_bring_the_divergence_down():
    z, y, x = _grid(16, 16, 16)
    v = np.stack([np.sin(x * 0.4) * np.cos(z * 0.3), 0.5 * np.cos(y * 0.35), np.sin(z * 0.25 + x * 0.2)], -1) * 0.3
    h = (1.0, 1.0, 1.0)
    l2 = lambda u: float(np.sqrt(np.mean(ref.divergence(u, h)[2:-2, 2:-2, 2:-2] ** 2)))  # noqa: E731
    after, _ = ref.project(v, h, 200)
    # The collocated projection (central gradient of a pressure solved with the compact Laplacian) cannot remove the
    # divergence altogether; on this smooth field the wide and the compact Laplacian differ by O(k^2 h^2) ~ 0.1: a factor 5
    assert l2(after) < l2(v) / 5.0
    one, _ = ref.project(v, h, 1)
    assert l2(after) < l2(one)


def test_boundary_factors_land_on_their_faces():
    shape = (7, 6, 8)
    one = np.ones(shape)
    s = ref.settings(boundary_damping=0.25)
    dens, temp, vel = ref.boundaries(one, one, np.ones(shape + (3,)), s)
    assert dens[3, 3, 0] == 0.58 and dens[3, 3, 7] == 0.58 and dens[3, 3, 1] == 0.78 and dens[3, 3, 6] == 0.78 and dens[3, 3, 3] == 1.0
    assert dens[0, 3, 3] == 0.58 and dens[6, 3, 3] == 0.58 and dens[1, 3, 3] == 0.78 and dens[5, 3, 3] == 0.78
    assert dens[3, 5, 3] == 1.0 and dens[3, 4, 3] == 1.0 and dens[3, 1, 3] == 1.0  # y loses nothing ...
    assert dens[3, 0, 3] == 0.75 and temp[3, 0, 3] == 0.75                          # ... but to the ground's damping
    assert temp[3, 3, 0] == 0.70 and temp[3, 3, 1] == 0.86 and temp[0, 3, 3] == 0.70 and temp[5, 3, 3] == 0.86
    assert dens[0, 3, 0] == pytest.approx(0.58 * 0.58) and dens[1, 3, 1] == pytest.approx(0.78 * 0.78) and dens[0, 0, 1] == pytest.approx(0.58 * 0.78 * 0.75)
    assert (vel[:, :, 0, 0] == 0).all() and (vel[:, :, -1, 0] == 0).all() and (vel[:, :, 1:-1, 0] == 1).all()
    assert (vel[:, 0, :, 1] == 0).all() and (vel[:, -1, :, 1] == 0).all() and (vel[:, 1:-1, :, 1] == 1).all()
    assert (vel[0, :, :, 2] == 0).all() and (vel[-1, :, :, 2] == 0).all() and (vel[1:-1, :, :, 2] == 1).all()
    dens, temp, _ = ref.boundaries(one, one, np.ones(shape + (3,)), ref.settings(boundary_damping=0.25, terrain_collision=False))
    assert dens[3, 0, 3] == 1.0 and temp[3, 0, 3] == 1.0


def test_grids_without_interior_pass_through_every_stencil():
    for dims in [(2, 2, 2), (3, 3, 3), (2, 5, 3)]:
        shape = dims[::-1]
        v = np.random.default_rng(4).normal(size=shape + (3,))
        assert ref.divergence(v, (1.0, 1.0, 1.0)).shape == shape
        out, len2 = ref.confine(v, (1.0, 1.0, 1.0), 0.4, 0.1)
        assert len2.size == 0 and np.array_equal(out, v)  # no margin-2 interior under 5 voxels an axis
    v = np.random.default_rng(4).normal(size=(5, 5, 5, 3))
    out, len2 = ref.confine(v, (1.0, 1.0, 1.0), 0.4, 0.1)
    assert len2.shape == (1, 1, 1) and (out != v).sum() == 3 and (out[2, 2, 2] != v[2, 2, 2]).all()


# ---- b. the oracle against the statement ----------------------------------------------------------------------------------------
def start_state(name):
    geo, emitters, settings, steps, seeder = cases.reference_sets()[name]
    st = so.new_state(sparse_threshold=cases.REFERENCE_THRESHOLD, **geo)
    seeder(st)
    return st, emitters, settings, steps


def compare_stepper(name, stepper, first_step=0, last_step=None, before=None):
    """Per field the largest residual and left-out share over the set's steps: the statement steps from `stepper`'s own state
    of the step before (through `before`, if given: what the altered steppers of part c do to the state first)."""
    st, emitters, settings, steps = start_state(name)
    s, em = ref.settings(**settings), [ref.emitter(**e) for e in emitters]
    worst = {f: (0.0, 0.0) for f in ref.FIELDS}
    for k in range(steps if last_step is None else last_step):
        if before is not None:
            before(st)
        want, masks = ref.step(ref.promote(st), s, em)
        stepper(st, emitters, settings)
        if k < first_step:
            continue
        assert st["frame_index"] == want["frame_index"] and abs(st["time_seconds"] - want["time_seconds"]) <= 4 * ref.EPS32 * want["time_seconds"]
        for f, (err, share) in ref.residuals(st, want, masks).items():
            worst[f] = (max(worst[f][0], err), max(worst[f][1], share))
    return worst


def _oracle_step(st, emitters, settings):
    so.step(st, emitters, steps=1, **settings)


@functools.lru_cache(maxsize=None)
def oracle_residuals(name):
    return compare_stepper(name, _oracle_step)


@pytest.mark.parametrize("name", sorted(cases.reference_sets()))
def test_oracle_equals_the_reference(name):
    worst = oracle_residuals(name)
    for f in ref.FIELDS:
        print(f"smoke-ref {name:26s} {f:14s} {worst[f][0]:8.2f} eps32*max|ref|   left out {worst[f][1]:.5f}")
    for f in ref.FIELDS:
        assert worst[f][1] <= ref.BAND_CAP, (name, f, worst[f][1])
    for f in ref.FIELDS:
        assert worst[f][0] <= ref.gate(name, f), (name, f, worst[f][0], ref.gate(name, f))


def test_every_set_has_smoke():
    """The sets are not trivial: smoke well over the threshold that is being aged, a finite flow."""
    for name in sorted(cases.reference_sets()):
        st, emitters, settings, steps = start_state(name)
        so.step(st, emitters, steps=steps, **settings)
        assert float(st["density"].max()) > 50 * cases.REFERENCE_THRESHOLD and np.isfinite(st["velocity"]).all(), name
        assert (st["particle_age"] >= 0).any(), name


# ---- c. the gate has teeth -------------------------------------------------------------------------------------------------------
TEETH_SET = "case-maccormack"  # dt = 0.2, hot emitters, 9 sweeps: every alteration moves its field by far more than rounding


def _fails(worst, name, fields):
    return [f for f in fields if worst[f][0] > ref.gate(name, f)]


def test_gate_catches_a_buoyancy_off_by_a_thousandth():
    def stepper(st, emitters, settings):
        so.step(st, emitters, steps=1, **{**settings, "buoyancy": so.STEP_DEFAULTS["buoyancy"] * (1.0 + 1e-3)})

    assert "velocity" in _fails(compare_stepper(TEETH_SET, stepper, last_step=2), TEETH_SET, ("velocity",))


def test_gate_catches_one_pressure_sweep_less():
    def stepper(st, emitters, settings):
        so.step(st, emitters, steps=1, **{**settings, "pressure_iterations": settings["pressure_iterations"] - 1})

    failed = _fails(compare_stepper(TEETH_SET, stepper, last_step=2), TEETH_SET, ("velocity", "pressure"))
    assert "velocity" in failed


def test_gate_catches_a_velocity_rolled_by_one_voxel():
    """The statement sees the state; the stepper steps the state with its velocity rolled one voxel along x."""
    pristine = {}

    def before(st):
        pristine["velocity"] = st["velocity"].copy()

    def stepper(st, emitters, settings):
        st["velocity"][...] = np.roll(pristine["velocity"], 1, axis=2)
        so.step(st, emitters, steps=1, **settings)

    assert "velocity" in _fails(compare_stepper(TEETH_SET, stepper, last_step=2, before=before), TEETH_SET, ("velocity",))


def test_the_unaltered_stepper_passes_where_the_altered_ones_fail():
    assert _fails(compare_stepper(TEETH_SET, _oracle_step, last_step=2), TEETH_SET, ref.FIELDS) == []
