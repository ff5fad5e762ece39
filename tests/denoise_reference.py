"""A float64 NumPy statement of the a-trous denoiser (csrc/f3d_denoise.h) -- TEST INFRASTRUCTURE ONLY.
Written from the operation's definition, not from oracle/denoise_oracle.py: a gather per tap with an explicit inside mask,
no shifted copies, so any tap spacing works (the arrays never grow with it) -- also spacings far beyond the image, where the
reference's own `_shift` refuses to answer (REFERENCE DOMAIN below).

The operation.  Inputs are float32 and promoted; everything after that is float64.
  * guide = albedo if given, else the ORIGINAL colour (never the iterate); normals are normalised once, v / max(1e-8, |v|)
  * max(1, iterations) passes; pass i has tap spacing 2^i
  * pass: out(p) = sum_t colour(p + t) w_t / max(sum_t w_t, 1e-8) over the 5 x 5 taps t = spacing * (dy, dx), dy, dx in -2..2
      w_t = k[dy] k[dx]                                   k = [1, 4, 6, 4, 1] / 16
            * exp(-|guide(p + t) - guide(p)|^2 / D_color)
            * exp(-|guide(p + t) - guide(p)|^2 / D_albedo)        only with an albedo and sigma_albedo > 0
            * exp(-acos(clip(n(p + t) . n(p), -1, 1))^2 / D_normal)     only with normals
            * exp(-(depth(p + t) - depth(p))^2 / D_depth)               only with a depth
      D_x = float32(2 sigma_x^2 + 1e-8): the ROUNDED divisor is part of the contract (inf for sigma = 1e20)
  * a tap outside the image reads 0 for the colour and for every guide, and its weight still counts in the normaliser
  * non-finite values follow NumPy's clip and maximum: a NaN is kept.

REFERENCE DOMAIN.  forge3d's `_shift` answers a shift o along an axis of n texels when o <= n (a real shift) or o >= 2 n
(nothing to copy) and raises ValueError ("could not broadcast") in between; a pass at spacing s shifts by s and by 2 s.
`reference_answers` says whether every pass of a call stays inside that; tests/golden/make_denoise_fixtures.py asserts that
the reference raises exactly where it says no.  In particular every call with 2 s <= min(H, W) in its last pass is answered.
Where the reference does not answer, this file is the contract.

TOLERANCES are measured, not chosen: MEASURED_ON_THE_ORACLE holds, per parameter set, the largest |float32 oracle - float64|
over all cases of the set (finite pixels), rounded up to two digits; the gate of a set is four times that (the project's
convention, tests/trace_reference.py: the device's expf / acosf are a few ulp where NumPy's are within one).  Print them with

    python -m pytest -m "not gpu" tests/test_denoise_host.py -k oracle -s | grep "denoise-ref"

Neither the host test nor the GPU test derives a tolerance from the code it checks.  Why the sets differ: the error is the
float32 rounding of an exponent's argument, |dg|^2 / D; the tighter the sigma, the larger the argument where the weight still
matters, and acos near 1 turns a 6e-8 rounding of n.n' into an angle of 3e-4 -- nothing against sigma_normal = 0.3, a
tenth of a tight 0.02 squared.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).resolve().parent / "golden"

MUTATIONS = ("outside_weights_dropped", "step_plus_one", "guide_is_iterate", "outside_reads_edge", "outside_guides_are_centre",
             "normals_not_normalised", "albedo_term_inverted", "no_pass_for_iterations_le_0", "width_height_exchanged")


def atrous_f64(color, *, albedo=None, normal=None, depth=None, iterations=3, sigma_color=0.1, sigma_albedo=0.2,
               sigma_normal=0.3, sigma_depth=0.5, mutate=None):
    """The denoised image, (H, W, 3) float64.  mutate: one of MUTATIONS -- a deliberately wrong variant (sensitivity test)."""
    assert mutate is None or mutate in MUTATIONS
    c = np.asarray(color, f32).astype(f64)
    h, w, _ = c.shape
    if mutate == "no_pass_for_iterations_le_0" and iterations <= 0:
        return c
    guide = c if albedo is None else np.asarray(albedo, f32).astype(f64)
    n = None
    if normal is not None:
        n = np.asarray(normal, f32).astype(f64)
        with np.errstate(all="ignore"):
            if mutate != "normals_not_normalised":
                n = n / np.maximum(1e-8, np.sqrt(np.sum(n * n, axis=-1, keepdims=True)))
    d = None if depth is None else np.asarray(depth, f32).astype(f64)
    with np.errstate(over="ignore"):
        D = {k: f64(f32(2.0 * float(s) ** 2 + 1e-8)) for k, s in (("color", sigma_color), ("albedo", sigma_albedo),
                                                                  ("normal", sigma_normal), ("depth", sigma_depth))}
    extra = albedo is not None and sigma_albedo > 0
    if mutate == "albedo_term_inverted":
        extra = albedo is not None and not sigma_albedo > 0
    k = np.array([1, 4, 6, 4, 1], f64) / 16.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    lim_y, lim_x = (w, h) if mutate == "width_height_exchanged" else (h, w)

    def gather(a, sy, sx, inside):
        v = a[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
        return np.where(inside if v.ndim == 2 else inside[..., None], v, 0.0)

    out, step = c, 1
    with np.errstate(all="ignore"):
        for _ in range(max(1, int(iterations))):
            g = out if (mutate == "guide_is_iterate" and albedo is None) else guide
            acc, wsum = np.zeros((h, w, 3), f64), np.zeros((h, w), f64)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    sy, sx = yy + dy * step, xx + dx * step
                    inside = (sy >= 0) & (sy < lim_y) & (sx >= 0) & (sx < lim_x)
                    seen = np.ones_like(inside) if mutate == "outside_reads_edge" else inside  # where a texel is read
                    dg = gather(g, sy, sx, seen) - g
                    gg = np.sum(dg * dg, axis=-1)
                    wt = k[dy + 2] * k[dx + 2] * np.exp(-gg / D["color"])
                    if extra:
                        wt = wt * np.exp(-gg / D["albedo"])
                    if n is not None:
                        m = gather(n, sy, sx, seen)
                        if mutate == "outside_guides_are_centre":
                            m = np.where(inside[..., None], m, n)
                        ang = np.arccos(np.clip(np.sum(m * n, axis=-1), -1.0, 1.0))
                        wt = wt * np.exp(-(ang * ang) / D["normal"])
                    if d is not None:
                        e = gather(d, sy, sx, seen)
                        if mutate == "outside_guides_are_centre":
                            e = np.where(inside, e, d)
                        wt = wt * np.exp(-((e - d) ** 2) / D["depth"])
                    # (an outside tap adds colour 0 times its weight: the product, so that 0 * NaN stays a NaN as in `_shift`'s sum)
                    acc += gather(out, sy, sx, seen) * wt[..., None]
                    wsum += np.where(inside, wt, 0.0) if mutate == "outside_weights_dropped" else wt
            out = acc / np.maximum(wsum, 1e-8)[..., None]
            step = step + 1 if mutate == "step_plus_one" else step * 2
    return out


def reference_answers(h, w, iterations):
    """Whether forge3d's NumPy implementation answers this call (REFERENCE DOMAIN above)."""
    for i in range(max(1, int(iterations))):
        for o in (1 << i, 2 << i):
            if any(n < o < 2 * n for n in (h, w)):
                return False
    return True


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# name -> what the set passes besides its inputs; "guides": which of the committed AOVs it takes
SETS = {
    "color_only": dict(guides=()),
    "all_guides": dict(guides=("albedo", "normal", "depth")),
    "normal_depth": dict(guides=("normal", "depth"), sigma_normal=0.1, sigma_depth=0.1),
    "albedo_no_extra": dict(guides=("albedo",), sigma_albedo=0.0),
    "tight": dict(guides=("albedo", "normal", "depth"), sigma_color=0.05, sigma_albedo=0.1, sigma_normal=0.1, sigma_depth=0.2),
    "very_tight": dict(guides=("albedo", "normal", "depth"), sigma_color=0.01, sigma_normal=0.02, sigma_depth=0.02),
    "sigma_color_0": dict(guides=(), sigma_color=0.0),
    "sigma_color_1e20": dict(guides=(), sigma_color=1e20),
    "color_wide": dict(guides=(), sigma_color=0.35),
    # on the dark image, with the depth scaled to 0.1: the only set in which a tap outside the image keeps a weight WITH guides
    # (elsewhere the zero depth or the zero albedo outside is so far from the centre's that the weight vanishes)
    "dark_guides": dict(guides=("normal", "depth"), sigma_color=0.35, sigma_normal=2.0, sigma_depth=0.5),
}
DEFAULT_SIGMA_SETS = ("color_only", "all_guides")

# largest |float32 oracle - float64| over the set's cases, rounded up to two digits (measured on the CPU; see the docstring)
MEASURED_ON_THE_ORACLE = {
    "color_only": 2.3e-6,  # color_only_17x15_it40 (2.28e-6; 40 passes)
    "all_guides": 4.1e-7,  # all_guides_33x31_it3
    "normal_depth": 6.1e-7,  # normal_depth_2 (40 x 52)
    "albedo_no_extra": 2.4e-7,  # albedo_no_extra_term (40 x 52)
    "tight": 1.8e-6,  # tight_33x31_it3
    "very_tight": 2.8e-5,  # very_tight_33x31_it3
    "sigma_color_0": 6.0e-8,  # one ulp of a value in [0.5, 1): the pass is centre * w / w
    "sigma_color_1e20": 1.1e-7,  # sigma_color_1e20_17x15_it3
    "dark_guides": 1.3e-8,  # dark_guides_17x15_it2 (values below 0.1: 3.5 ulp)
    "color_wide": 4.2e-7,  # color_only_1_wide (40 x 52)
}
TOL = {k: 4.0 * v for k, v in MEASURED_ON_THE_ORACLE.items()}
OLD_TOL = 2e-5  # the gate of tests/test_denoise.py; every default-sigma set must come out below it
assert all(TOL[k] < OLD_TOL for k in DEFAULT_SIGMA_SETS)

# mutation -> (the case that must move by at least 100 x its tolerance, the largest move over ALL finite cases as measured
# by `python tests/denoise_reference.py`, the case it was seen on)
SENSITIVITY = {
    "outside_weights_dropped": (("sigma_color_1e20_3x5_it3", "dark_border_17x15_it2"), 0.907, "sigma_color_1e20_3x5_it3"),
    "step_plus_one": (("sigma_color_1e20_17x15_it3",), 0.194, "sigma_color_1e20_17x15_it3"),
    "guide_is_iterate": (("normal_depth_16x16_it3",), 0.0414, "normal_depth_16x16_it3"),
    "outside_reads_edge": (("sigma_color_1e20_1x7_it3",), 0.935, "sigma_color_1e20_1x7_it3"),
    "outside_guides_are_centre": (("dark_guides_17x15_it2",), 0.00524, "dark_guides_17x15_it2"),
    "normals_not_normalised": (("all_guides_17x15_it7",), 0.0909, "all_guides_17x15_it7"),
    "albedo_term_inverted": (("albedo_no_extra_16x16_it3",), 0.15, "albedo_no_extra_16x16_it3"),
    "no_pass_for_iterations_le_0": (("all_guides_3x5_it-3",), 0.171, "all_guides_3x5_it-3"),
    "width_height_exchanged": (("sigma_color_0_1x7_it3",), 1.12, "sigma_color_0_1x7_it3"),
}
assert set(SENSITIVITY) == set(MUTATIONS)

SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (16, 16), (17, 15), (33, 31), (40, 52))
NONFINITE = {  # on 17 x 15, two passes: name -> (set, the array poked, index, value)
    "nan_normal_component": ("all_guides", "normal", (7, 6, 1), np.nan),
    "nan_normal_whole": ("all_guides", "normal", (0, 14), np.nan),
    "inf_normal": ("all_guides", "normal", (7, 6, 0), np.inf),
    "nan_depth": ("all_guides", "depth", (7, 6), np.nan),
    "inf_depth": ("all_guides", "depth", (16, 0), np.inf),
    "inf_colour": ("color_only", "color", (7, 6, 0), np.inf),
    "nan_albedo": ("all_guides", "albedo", (7, 6, 2), np.nan),
}


def _case(name, pset, h, w, iterations, **more):
    return dict(name=name, set=pset, shape=(h, w), iterations=iterations, **more)


def cases():
    """The table: every parameter set on every small shape, the iteration counts where a pass count changes the path, the dark
    border, the non-finite inputs, and the seven committed 40 x 52 cases (whose reference vectors are in atrous_cases.npz)."""
    out = []
    for pset in SETS:
        if pset in ("color_wide", "dark_guides"):  # (the dark border and the committed wide case below)
            continue
        for h, w in SHAPES[:6]:  # below the 5 x 5 footprint, the exact block, one past / one short of it
            out.append(_case(f"{pset}_{h}x{w}_it3", pset, h, w, 3))
    for pset in ("color_only", "all_guides", "tight", "very_tight"):  # several blocks, ragged on both axes
        out.append(_case(f"{pset}_33x31_it3", pset, 33, 31, 3))
    for pset, its in (("color_only", (-3, 0, 2, 7, 40)), ("all_guides", (1, 2, 7, 40))):
        for it in its:
            out.append(_case(f"{pset}_17x15_it{it}", pset, 17, 15, it))
    for h, w in ((1, 1), (3, 5)):  # every tap but the centre outside from the first or second pass on
        for it in (-3, 0, 1, 2, 7):
            out.append(_case(f"all_guides_{h}x{w}_it{it}", "all_guides", h, w, it))
    for h, w in ((1, 7), (7, 1)):  # a line: one axis always outside, the other inside the reference's domain
        out.append(_case(f"all_guides_{h}x{w}_it2", "all_guides", h, w, 2))
    out.append(_case("dark_border_17x15_it2", "color_wide", 17, 15, 2, dark=True))
    out.append(_case("dark_border_3x5_it1", "color_wide", 3, 5, 1, dark=True))
    # passes 6 and 7: every tap but the centre outside and still weighty -- centre * 0.140625 / sum(w), far from the identity
    out.append(_case("dark_border_17x15_it7", "color_wide", 17, 15, 7, dark=True))
    out.append(_case("dark_guides_17x15_it2", "dark_guides", 17, 15, 2, dark=True))
    out.append(_case("dark_guides_3x5_it1", "dark_guides", 3, 5, 1, dark=True))
    for name, (pset, _, _, _) in NONFINITE.items():
        out.append(_case(f"{name}_17x15_it2", pset, 17, 15, 2, poke=name))
    for name, pset, it in (("color_only_3", "color_only", 3), ("color_only_1_wide", "color_wide", 1), ("all_guides_3", "all_guides", 3),
                           ("all_guides_4_tight", "tight", 4), ("normal_depth_2", "normal_depth", 2),
                           ("albedo_no_extra_term", "albedo_no_extra", 2), ("zero_iterations_means_one", "color_only", 0)):
        out.append(_case(name, pset, 40, 52, it, committed=True))
    assert len({c["name"] for c in out}) == len(out)
    return out


_BASE = None


def base():
    """The committed 40 x 52 inputs, their reference vectors, and the edge file when it exists."""
    global _BASE
    if _BASE is None:
        z = np.load(GOLDEN / "atrous_cases.npz")
        _BASE = {k: z[k] for k in z.files}
        edge = GOLDEN / "atrous_edge_cases.npz"
        if edge.exists():
            z = np.load(edge)
            _BASE.update({k: z[k] for k in z.files})
    return _BASE


def dark_image():
    """17 x 15 from uniform(0, 0.1): so dark that an outside tap (colour 0) weighs almost what an inside one does."""
    return np.random.default_rng(20261020).uniform(0.0, 0.1, (17, 15, 3)).astype(f32)


def inputs(case, dark=None):
    """(colour, keyword arguments) of a case: crops of the committed inputs from their top-left corner; float32, C order.
    dark: the dark image (the generator passes a fresh one; the tests read the one the edge file carries)."""
    b = base()
    h, w = case["shape"]
    if case.get("dark"):
        color = (b["dark_color"] if dark is None else dark)[:h, :w]
    else:
        color = b["color"][:h, :w]
    arrays = {"color": np.ascontiguousarray(color, f32).copy()}
    spec = SETS[case["set"]]
    for g in spec["guides"]:
        arrays[g] = np.ascontiguousarray(b[g][:h, :w], f32).copy()
        if g == "depth" and case.get("dark"):
            arrays[g] *= f32(0.01)
    if case.get("poke"):
        _, which, idx, value = NONFINITE[case["poke"]]
        arrays[which][idx] = value
    kw = {k: v for k, v in spec.items() if k != "guides"}
    kw.update({g: arrays[g] for g in spec["guides"]}, iterations=case["iterations"])
    return arrays["color"], kw


def golden(case):
    """The reference's own output for the case, or None where the reference does not answer."""
    b = base()
    key = "want_" + case["name"]
    if not reference_answers(*case["shape"], case["iterations"]):
        assert key not in b
        return None
    return b[key]


_WANT = {}


def want(case):
    """atrous_f64 of the case, computed once and shared (read-only)."""
    if case["name"] not in _WANT:
        color, kw = inputs(case)
        r = atrous_f64(color, **kw)
        r.setflags(write=False)
        _WANT[case["name"]] = r
    return _WANT[case["name"]]


def gate(case, got, golden_vector=None):
    """The gates of a case on a float32 result.  Returns (largest error on the finite pixels, tolerance); raises AssertionError."""
    ref = want(case)
    tol = TOL[case["set"]]
    name = case["name"]
    assert got.dtype == f32 and got.shape == ref.shape, name
    bad = ~np.isfinite(ref)
    assert np.array_equal(~np.isfinite(got), bad), (name, "non-finite pixels", int((~np.isfinite(got)).sum()), int(bad.sum()))
    if golden_vector is not None:
        assert np.array_equal(~np.isfinite(golden_vector), bad), (name, "non-finite pixels of the reference's vector")
    if bad.any():  # NaN or Inf, the same one
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[bad & ~np.isnan(ref)], ref[bad & ~np.isnan(ref)]), name
    err = float(np.abs(got.astype(f64) - ref)[~bad].max()) if (~bad).any() else 0.0
    assert err <= tol, (name, err, tol)
    return err, tol


def oracle_error(case, oracle_result):
    ref = want(case)
    ok = np.isfinite(ref)
    return float(np.abs(oracle_result.astype(f64) - ref)[ok].max()) if ok.any() else 0.0


def mutation_move(case, mutation):
    """Largest |mutated - float64| of a finite case, as a multiple of the case's tolerance."""
    color, kw = inputs(case)
    return float(np.abs(atrous_f64(color, **kw, mutate=mutation) - want(case)).max()) / TOL[case["set"]]


if __name__ == "__main__":  # the sensitivity table over all finite cases
    finite = [c for c in cases() if not c.get("poke")]
    for m in MUTATIONS:
        moves = [(float(np.abs(atrous_f64(inputs(c)[0], **inputs(c)[1], mutate=m) - want(c)).max()), c) for c in finite]
        best = max(moves, key=lambda t: t[0] / TOL[t[1]["set"]])
        print(f"{m:30s} {best[0]:.3g} = {best[0] / TOL[best[1]['set']]:.3g} x tol on {best[1]['name']}")
