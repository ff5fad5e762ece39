"""The HIP smoke ray-marcher (SmokeDomain.render_rgba / render_projection_rgba, csrc/f3d_smoke.hip) against the float64 statement
of a ray (tests/smoke_march_reference.py): every set of tests/smoke_march_cases.py in the three forms of the device marcher,
under the 8-bit gate and the bias gate derived from the float gates that were measured on the oracle's float march
(tests/test_smoke_march_reference_host.py), with the reference's masks and its cap.  No oracle, no emulator."""
from __future__ import annotations

import numpy as np
import pytest

import smoke_march_cases as cases
import smoke_march_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    """A set's reference image, computed once for the three forms."""
    images = {}

    def get(name):
        if name not in images:
            s = cases.reference_sets()[name]
            w, h = s["size"]
            view = dict(view_direction=s["view"]) if s["projection"] else dict(**s["camera"])
            vol = ref.volume(s["fields"], voxel_size=s["voxel_size"], origin=s["origin"], frame_index=s["frame_index"])
            images[name] = ref.render(vol, w, h, ref.settings(**s["settings"]), s["sun"], projection=s["projection"], **view)
        return images[name]

    return get


def _domain(s):
    from forge3d_amd import smoke

    f = s["fields"]
    d = f["density"]
    dom = smoke.SmokeDomain((d.shape[2], d.shape[1], d.shape[0]), s["voxel_size"], s["origin"])
    dom.set_density(d)
    for name, setter in (("temperature", dom.set_temperature), ("soot", dom.set_soot), ("humidity", dom.set_humidity), ("emission_rate", dom.set_emission)):
        if name in f:
            setter(f[name])
    dom.set_particle_age(f["particle_age"] if "particle_age" in f else np.full(d.shape, -1.0, np.float32))
    dom.frame_index = s["frame_index"]
    return dom


@pytest.mark.parametrize("form", ["deferred", "deferred-short-list", "single"])
@pytest.mark.parametrize("name", list(cases.reference_sets()))
def test_hip_marcher_equals_the_reference(name, form, want, monkeypatch):
    from forge3d_amd import smoke

    monkeypatch.delenv("F3D_SMOKE_MARCH", raising=False)
    monkeypatch.delenv("F3D_SMOKE_SHADOW_SLOTS", raising=False)
    if form == "single":
        monkeypatch.setenv("F3D_SMOKE_MARCH", form)
    elif form == "deferred-short-list":
        monkeypatch.setenv("F3D_SMOKE_SHADOW_SLOTS", "3072")
    s = cases.reference_sets()[name]
    image = want(name)
    assert ref.masked_share(image) <= ref.MASK_CAP
    args, kw = cases.render_args(name)
    dom = _domain(s)
    render = dom.render_projection_rgba if s["projection"] else dom.render_rgba
    got = render(*args, **kw, settings=smoke.SmokeRenderSettings(**s["settings"]))
    assert got.shape == image["alpha"].shape + (4,) and got.dtype == np.uint8
    ref.hold_codes(name, form, got, image)
