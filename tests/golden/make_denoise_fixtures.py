#!/usr/bin/env python
"""Golden vectors of the a-trous denoiser, produced by the REFERENCE's own NumPy implementation
(python/forge3d/denoise.py is pure NumPy and importable in the build container; the native module is
not needed).  Run here only -- /root/reference does not exist on the GPU box; the .npz travels.

    PYTHONPATH=/root/reference/python python tests/golden/make_denoise_fixtures.py

Writes atrous_cases.npz (if it is not there; otherwise checks that it holds what this script computes) and
atrous_edge_cases.npz.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

spec = importlib.util.spec_from_file_location("ref_denoise", "/root/reference/python/forge3d/denoise.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

rng = np.random.default_rng(20260927)
h, w = 40, 52
yy, xx = np.mgrid[0:h, 0:w]
clean = np.stack([0.5 + 0.4 * np.sin(xx / 7.0), 0.5 + 0.4 * np.cos(yy / 5.0), np.where(xx > w // 2, 0.9, 0.2)], -1)
color = np.clip(clean + rng.normal(0, 0.08, clean.shape), 0, 1.5).astype(np.float32)
albedo = np.stack([np.where(xx > w // 2, 0.8, 0.3), np.where(yy > h // 3, 0.6, 0.5), 0.4 + 0.0 * xx], -1).astype(np.float32)
normal = np.stack([np.sin(xx / 9.0), np.cos(yy / 11.0) * 0.5, 1.0 + 0.0 * xx], -1).astype(np.float32)  # not unit length
normal[3, 4] = 0.0  # a zero normal: the eps branch of the normalisation
depth = (10.0 + 0.05 * xx + np.where(yy > h // 2, 3.0, 0.0) + rng.normal(0, 0.01, (h, w))).astype(np.float32)
cases = {
    "color_only_3": dict(iterations=3),
    "color_only_1_wide": dict(iterations=1, sigma_color=0.35),
    "all_guides_3": dict(albedo=albedo, normal=normal, depth=depth, iterations=3),
    "all_guides_4_tight": dict(albedo=albedo, normal=normal, depth=depth, iterations=4, sigma_color=0.05,
                               sigma_albedo=0.1, sigma_normal=0.1, sigma_depth=0.2),
    "normal_depth_2": dict(normal=normal, depth=depth, iterations=2, sigma_normal=0.1, sigma_depth=0.1),
    "albedo_no_extra_term": dict(albedo=albedo, iterations=2, sigma_albedo=0.0),
    "zero_iterations_means_one": dict(iterations=0),
}
out = {"color": color, "albedo": albedo, "normal": normal, "depth": depth}
for name, kw in cases.items():
    out["want_" + name] = ref.atrous_denoise(color, **kw)
here = Path(__file__).resolve().parent
if (here / "atrous_cases.npz").exists():  # the committed file stays byte for byte (a .npz carries the time it was written)
    z = np.load(here / "atrous_cases.npz")
    assert sorted(z.files) == sorted(out) and all(np.array_equal(z[k], v) for k, v in out.items()), "atrous_cases.npz is not what this script writes"
else:
    np.savez_compressed(here / "atrous_cases.npz", **out)
print({k: v.shape for k, v in out.items()})

# ---- atrous_edge_cases.npz: the reference's outputs for the case table of tests/denoise_reference.py, wherever the reference
# answers (the non-finite inputs included: the NaN contract is then the reference's own), and the dark image of the border case.
# Where tests/denoise_reference.py says the reference does not answer, it must raise: its `_shift` cannot form the shift.
sys.path.insert(0, str(here.parent))
import denoise_reference as dr  # noqa: E402

dark = dr.dark_image()
edge, refused = {"dark_color": dark}, []
with np.errstate(all="ignore"):
    for case in dr.cases():
        if case.get("committed"):
            continue
        c, kw = dr.inputs(case, dark)
        if dr.reference_answers(*case["shape"], case["iterations"]):
            edge["want_" + case["name"]] = ref.atrous_denoise(c, **kw)
        else:
            try:
                ref.atrous_denoise(c, **kw)
            except ValueError as e:
                assert "could not broadcast" in str(e), e
                refused.append(case["name"])
            else:
                raise AssertionError(case["name"] + ": the reference answered outside the domain denoise_reference.py states")
np.savez_compressed(here / "atrous_edge_cases.npz", **edge)
size = (here / "atrous_edge_cases.npz").stat().st_size
assert size < (here / "atrous_cases.npz").stat().st_size, size
print(f"atrous_edge_cases.npz: {len(edge) - 1} vectors, {size} bytes; the reference refused {len(refused)} cases: {refused}")
