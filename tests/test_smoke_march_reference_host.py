"""The float64 statement of a smoke ray (tests/smoke_march_reference.py) and the oracle held to it -- no GPU.

a. known answers of the reference itself, term by term (closed forms, hand-computed hashes, the reference's four unit tests);
b. the oracle's float march (smoke_oracle.hook_march) against the reference per set and channel, in eps32 of the channel's
   largest value, under gates that are four times what MEASURED_ON_THE_ORACLE records; equal step counts; the mask cap;
c. every constant of the reference's table, and three structural choices, perturbed one at a time: some set must fail (b);
d. the oracle's 8-bit images under the derived 8-bit gate and the bias gate."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import smoke_march_cases as cases
import smoke_march_reference as ref
from oracle import smoke_oracle

SETS = list(cases.reference_sets())


def _geometry(s):
    return dict(voxel_size=s["voxel_size"], origin=s["origin"], frame_index=s["frame_index"])


def _reference(name, K=ref.CONSTANTS, S=ref.STRUCTURE):
    s = cases.reference_sets()[name]
    w, h = s["size"]
    view = dict(view_direction=s["view"]) if s["projection"] else dict(**s["camera"])
    return ref.render(ref.volume(s["fields"], **_geometry(s)), w, h, ref.settings(**s["settings"]), s["sun"], projection=s["projection"], K=K, S=S, **view)


@functools.lru_cache(maxsize=None)
def _want(name):
    return _reference(name)


@functools.lru_cache(maxsize=None)
def _oracle_floats(name):
    s = cases.reference_sets()[name]
    w, h = s["size"]
    view = dict(view_direction=s["view"]) if s["projection"] else dict(**s["camera"])
    return smoke_oracle.hook_march(s["fields"], w, h, projection=s["projection"], sun_direction=s["sun"], **view, **_geometry(s), **s["settings"])


def _oracle_bytes(name):
    s = cases.reference_sets()[name]
    args, kw = cases.render_args(name)
    render = smoke_oracle.render_projection_rgba if s["projection"] else smoke_oracle.render_rgba
    return render(s["fields"], *args, **kw, **_geometry(s), **s["settings"])


# ---- a. known answers of the reference ------------------------------------------------------------------------------------------
def test_an_empty_volume_renders_nothing():
    vol = ref.volume({"density": np.zeros((6, 5, 7), np.float32)})
    for kw in (dict(camera_pos=(3.3, 2.2, -9.0), target=(3.4, 2.6, 3.1)), dict(projection=True, view_direction=(0.1, -1.0, 0.2))):
        img = ref.render(vol, 9, 7, ref.settings(), cases.SUN, **kw)
        assert not img["rgb"].any() and not img["alpha"].any() and (img["transmittance"] == 1.0).all()
        assert img["steps"].max() > 0  # the rays do walk the box


def test_a_uniform_slab_absorbs_in_closed_form():
    """Extinction alone: density 1 everywhere (gate 1, no age, no soot), no jitter, a vertical projection through 8 units in steps
    of 0.3: 27 steps (t_26 = 7.8 < 8 <= t_27), each exp(-sigma * 0.3), so alpha = 1 - exp(-sigma * 27 * 0.3)."""
    vol = ref.volume({"density": np.ones((6, 8, 5), np.float32)})
    st = ref.settings(step_size=0.3, jitter_strength=0.0, self_shadow=False, extinction=0.2, density_scale=1.5, max_steps=100)
    img = ref.render(vol, 4, 3, st, cases.SUN, projection=True, view_direction=(0.0, -1.0, 0.0))
    sigma = 1.5 * float(np.float32(0.2))  # T = exp(-2.43): well above the opacity cut-off
    h = float(np.float32(0.3))
    assert (img["steps"] == 27).all() and not img["masked"].any()
    assert np.allclose(img["alpha"], 1.0 - math.exp(-sigma * 27 * h), rtol=1e-13, atol=0)
    assert np.allclose(img["transmittance"], math.exp(-sigma * 27 * h), rtol=1e-13, atol=0)


def test_sun_transmittance_through_a_uniform_block_in_closed_form():
    """exp(-sigma' L) with the self-shadow march's own sigma' = d * scale * extinction * (1 + soot * soot_absorption): no 0.85.
    From x = 3.2 along +x in steps of 0.7 through a 24-wide box: the march starts at 3.9, t1 = 20.1, samples at (i + 0.5) * 0.7
    <= 20.1, i = 0 ... 28: L = 29 * 0.7."""
    shape = (6, 6, 24)
    vol = ref.volume({"density": np.full(shape, 0.5, np.float32), "soot": np.full(shape, 0.5, np.float32)})
    st = ref.settings(extinction=0.4, soot_absorption=0.6, density_scale=1.0)
    f = lambda v: float(np.float32(v))  # noqa: E731
    sigma = 0.5 * f(0.4) * (1.0 + 0.5 * f(0.6))
    got = ref.sun_transmittance(vol, [(3.2, 2.9, 3.1)], (1.0, 0.0, 0.0), 0.7, 48, st)
    assert np.allclose(got, math.exp(-sigma * 29 * f(0.7)), rtol=1e-13, atol=0)
    with_ray_factor = math.exp(-0.5 * f(0.4) * (1.0 + 0.5 * f(0.6) * 0.85) * 29 * f(0.7))
    assert abs(float(got[0]) - with_ray_factor) > 0.05 * float(got[0])  # the ray's 0.85 here would be a 20 % error
    assert float(ref.sun_transmittance(vol, [(3.2, 2.9, 3.1)], (1.0, 0.0, 0.0), 0.7, 5, st)[0]) == pytest.approx(math.exp(-sigma * 5 * f(0.7)), rel=1e-13)
    dense = ref.volume({"density": np.full(shape, 3.0, np.float32)})  # od passes 8 at the 10th step and stays there: 10 * 0.84
    assert float(ref.sun_transmittance(dense, [(3.2, 2.9, 3.1)], (1.0, 0.0, 0.0), 0.7, 48, st)[0]) == pytest.approx(math.exp(-3.0 * f(0.4) * f(0.7) * 10), rel=1e-12)


def test_smoke_color_single_colour_limits():
    st = ref.settings()
    zero = np.zeros(1)
    thin = ref.smoke_color(zero, zero, zero, zero, zero, st)
    assert np.array_equal(thin[0], st["thin_color"])  # body = 0, young, dry, cold
    dense = ref.smoke_color(np.ones(1), zero, zero, zero, zero, st)
    assert np.allclose(dense[0], st["dense_color"], rtol=1e-15)  # body = 1 (clamped from 1.45)
    old = ref.smoke_color(zero, zero, zero, zero, np.full(1, 30.0), st)  # aged fully: 0.42 of the way to the aged grey
    assert np.allclose(old[0], st["thin_color"] + (np.array([0.36, 0.39, 0.43]) - st["thin_color"]) * 0.42, rtol=1e-15)


def test_jitter_hash_against_hand_computed_seeds():
    """The two multiply-xorshift rounds by hand (plain integers): seed -> 32-bit hash."""
    for seed, hashed in ((0, 0), (1, 1753845952), (260267682, 323857578), (910384804, 4085949223)):
        assert float(ref.hash01(np.array([seed]))[0]) == hashed / 4294967296.0
    assert int(ref.jitter_seed(3, 2, 77, False)) == 3 * 73856093 + 2 * 19349663 + 77 == 260267682
    assert int(ref.jitter_seed(60, 40, 0, False)) == 910384804  # 5205352100 wrapped
    assert int(ref.jitter_seed(60, 40, 5, True)) == 3564820578


def test_default_step_sizes():
    vol = ref.volume({"density": np.zeros((4, 4, 4), np.float32)}, voxel_size=(2.0, 1.5, 2.5))
    assert ref.step_sizes(vol, ref.settings()) == (1.5 * 0.75, 1.5 * 0.75 * 2.0)
    assert ref.step_sizes(vol, ref.settings(step_size=0.5, shadow_step_size=0.25)) == (0.5, 0.25)
    tiny = ref.volume({"density": np.zeros((4, 4, 4), np.float32)}, voxel_size=(5e-5, 1.0, 1.0))  # the floor of 1e-4 under the voxel
    assert ref.step_sizes(tiny, ref.settings())[0] == 1.0e-4 * 0.75


def test_the_references_unit_tests_hold_of_the_float64_statement():
    """render.rs:426-591, the four properties tests/test_smoke.py holds the oracle to, here on the reference (codes = 255 v)."""
    fields = {"density": cases.ball((16, 16, 16), (8, 8, 8), 4.0, 4.0), "temperature": cases.ball((16, 16, 16), (8, 8, 8), 4.0, 1.0)}
    fields["particle_age"] = np.where(fields["density"] > 0, 0.0, -1.0).astype(np.float32)
    img = ref.render(ref.volume(fields), 32, 32, ref.settings(), cases.SUN, camera_pos=(8.0, 8.0, -18.0), target=(8.0, 8.0, 8.0))
    assert img["alpha"].max() * 255 > 1 and img["alpha"][0, 0] == 0.0

    img = ref.render(ref.volume({"density": cases.ball((14, 12, 18), (8, 4, 7), 3.5, 5.0)}), 36, 28, ref.settings(), cases.SUN, projection=True)
    ys, xs = np.nonzero(img["alpha"] * 255 > 128)
    assert abs(xs.mean() / 36 - 8 / 18) < 0.08 and abs(ys.mean() / 28 - 7 / 14) < 0.08

    density = np.zeros((12, 12, 24), np.float32)
    density[3:9, 3:9, 8:14] = 1.2
    vol = ref.volume({"density": density, "soot": (density * 0.15).astype(np.float32)})
    st = ref.settings(density_scale=1.4, extinction=1.8)
    lit = ref.sun_transmittance(vol, [(15.0, 6.0, 6.0)], (1.0, 0.0, 0.0), 0.5, 48, st)[0]
    occluded = ref.sun_transmittance(vol, [(15.0, 6.0, 6.0)], (-1.0, 0.0, 0.0), 0.5, 48, st)[0]
    assert lit > 0.95 and occluded < 0.35

    density = np.zeros((16, 16, 16), np.float32)
    density[5:11, 5:11, 5:11] = 0.55
    hot = {"density": density, "temperature": np.where(density > 0, 0.85, 0).astype(np.float32), "emission_rate": np.where(density > 0, 1.4, 0).astype(np.float32)}
    st = ref.settings(density_scale=1.2, extinction=1.25, fire_glow=1.25, exposure=1.15)
    cam = dict(camera_pos=(8.0, 8.0, -18.0), target=(8.0, 8.0, 8.0))
    with_e = ref.render(ref.volume(hot), 32, 32, st, (0.3, 0.8, -0.2), **cam)["rgb"] * 255
    without = ref.render(ref.volume({"density": density}), 32, 32, st, (0.3, 0.8, -0.2), **cam)["rgb"] * 255
    assert (with_e[..., 0] - with_e[..., 2]).max() > (without[..., 0] - without[..., 2]).max() + 12
    assert with_e[..., 0].max() > without[..., 0].max()


# ---- b. the oracle's float march against the reference ----------------------------------------------------------------------------
def _fails_its_gate(name, want):
    r = ref.residuals(_oracle_floats(name), want)
    return r["steps"] > 0 or any(r[ch] > ref.gate(name, ch) for ch in ref.CHANNELS)


@pytest.mark.parametrize("name", SETS)
def test_oracle_float_march_equals_the_reference(name):
    want = _want(name)
    share = ref.masked_share(want)
    solid = int((~want["faint"]).sum())
    print(f"smoke-march-ref {name:18s} masks: " + ", ".join(f"{k} {int(m.sum())}" for k, m in want["reasons"].items()) + f"; left out {share:.4f} of {solid} pixels above the alpha floor")
    assert share <= ref.MASK_CAP, (name, share)  # of the reference alone
    assert solid >= 8 and want["alpha"].max() > 0.9  # the set shows smoke, up to opaque
    r = ref.residuals(_oracle_floats(name), want)
    for ch in ref.CHANNELS:
        print(f"smoke-march-ref {name:18s} {ch:14s} {r[ch]:8.2f} eps32*max|ref|   recorded {ref.MEASURED_ON_THE_ORACLE[name][ch]:g}, gate {ref.gate(name, ch):g}")
    assert r["steps"] == 0, (name, r["steps"])
    for ch in ref.CHANNELS:
        assert r[ch] <= ref.gate(name, ch), (name, ch, r[ch], ref.gate(name, ch))
        assert ref.gate(name, ch) <= 4.0 * ref.MEASURED_ON_THE_ORACLE[name][ch] * 1.1  # the gate is four times a recorded value, rounded up


def test_the_sets_reach_what_they_are_named_for():
    """The ends the table of sets promises, read off the reference's result."""
    cut = _want("cut")
    assert (cut["steps"] == 14).sum() > 50 and cut["steps"].max() == 14  # rays cut inside the smoke
    dense = _want("sooty-dense")
    assert ((dense["transmittance"] <= 0.01) & (dense["transmittance"] > 0)).sum() > 50  # rays that end at the opacity cut-off
    assert _want("thin")["alpha"].shape == (3, 5) and cases.reference_sets()["thin"]["fields"]["density"].shape[1] == 2
    assert (_want("inside")["alpha"] > 0).mean() > 0.9  # the camera sits in smoke


# ---- c. every constant is seen ----------------------------------------------------------------------------------------------------
# Which set to try first (any set may catch it; this only saves time).
SEEN_BY = {"plane_height": "projection-oblique", "albedo_lo": "sooty-dense", "sky_soot_lo": "sooty-dense", "milk_clamp": "sooty-dense",
           "albedo_hi": "cut", "bounce_min_height": "thin", "fire_clamp": "emitting", "fire_b": "emitting", "tint_fresh": "aged-humid",
           "density_floor": "projection", "shadow_step_ratio": "sooty-dense", "step_fraction": "aged-humid", "phase_power": "thin",
           "bounce_from_floor": "awkward-voxel", "min_step": "tiny-voxel"}

# A 1 % change of these cannot move a compared pixel by a float32 rounding, in any volume under validated settings; each with
# its derivation.  (The floor under the default step is NOT one of them: the set "tiny-voxel" has voxel edges under it.)
EXEMPT = {
    "parallel": "1 / d replaced by inf for |d| <= 1e-12: a 1 % change matters to a unit direction with a component in (1e-12, 1.01e-12], "
                "where 1 / d >= 9.9e11 already puts that slab's planes beyond every other plane of a box of any size a float32 grid can have",
    "sigma_floor": "the segment weight is `step` below it and (1 - exp(-s h)) / s = h (1 - s h / 2 + ...) above it: at s = 1e-6 the two "
                   "differ by s h / 2 < 1e-6 h, and a 1 % move of the switch picks between them only for s in (1e-6, 1.01e-6]",
    "phase_floor": "validated settings have |g| <= 0.99, so the denominator 1 + g^2 - 2 g cos >= (1 - |g|)^2 >= 1e-4 (1 - 2e-6): the floor "
                   "acts only within 2e-6 (relative) of itself, for cos within 1e-6 of +-1",
    "alpha_switch": "rgb / alpha above it, rgb below it: pixels with alpha within 2e-6 of 1e-5 are masked (\"unpremultiply\"), and a 1 % move of the "
                    "switch, to 1.01e-5, stays inside that band; every pixel near it is under the alpha floor anyway, where colour is compared "
                    "premultiplied and both branches give a colour * alpha below 1e-5 of a code",
    "smooth_floor": "the floor under a smoothstep's width e1 - e0: render.rs calls it with the literal edges (1.6, 17) and (0.045, 0.34) only, "
                    "widths 15.4 and 0.295, so max(width, 1e-6) is the width for any volume and any settings",
    "albedo_eps": "1e-5 added to scattering + absorption + 0.55 soot in the albedo's denominator: 1 % of it is 1e-7 against a denominator "
                  "of order 1, i.e. 1e-7 of the albedo, under an eps32; it matters only where all three are 0, which validate() allows but "
                  "no smoke has (then the albedo is 0 / 1e-5 = 0, clamped to 0.02 either way)",
}


def _sets_in_order(first):
    return ([first] if first else []) + [n for n in SETS if n != first]


@pytest.mark.parametrize("key", list(ref.CONSTANTS))
def test_a_one_percent_change_of_a_constant_fails_some_set(key):
    if key in EXEMPT:
        assert len(EXEMPT[key]) > 60  # a derivation, not a shrug
        K = {**ref.CONSTANTS, key: ref.CONSTANTS[key] * 1.01}
        assert not any(_fails_its_gate(name, _reference(name, K=K)) for name in ("plume", "cut"))  # and indeed unseen
        return
    K = {**ref.CONSTANTS, key: ref.CONSTANTS[key] * 1.01}
    assert any(_fails_its_gate(name, _reference(name, K=K)) for name in _sets_in_order(SEEN_BY.get(key, "inside"))), f"no set sees {key}"


@pytest.mark.parametrize("key", list(ref.STRUCTURE))
def test_a_structural_mutation_fails_some_set(key):
    """The 0.85 applied in the self-shadow march too; p.y measured from the domain's floor in the bounce term; t0 not clamped at 0."""
    S = {**ref.STRUCTURE, key: not ref.STRUCTURE[key]}
    assert any(_fails_its_gate(name, _reference(name, S=S)) for name in _sets_in_order(SEEN_BY.get(key, "inside"))), f"no set sees {key}"


def test_the_unmutated_reference_fails_no_set():
    assert not any(_fails_its_gate(name, _want(name)) for name in SETS)


# ---- d. the 8-bit images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_oracle_images_equal_the_reference_to_the_rounding(name):
    ref.hold_codes(name, "oracle", _oracle_bytes(name), _want(name))
