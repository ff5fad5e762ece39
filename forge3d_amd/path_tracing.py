"""Public entry point of the terrain path tracer: ``hybrid_render_terrain_reference``.

The CONTRACT is the reference's (python/forge3d/path_tracing.py:893-929 signature; :970-1001 validation
order, exception types and message texts; :1092-1094 the three sun keys added to the result) and is pinned
by tests/golden/wrapper_contract.json, captured from the reference package.  The implementation is this
package's own: the call is normalised into a ``_Request`` (arrays coerced once, options kept by name), an
ordered rule table rejects bad input before any device work, the sun is resolved by ``_SunResolution`` and
the native keyword set is produced from a conversion table.  The render runs in ``forge3d_amd._native`` ->
libf3dhip.so -> HIP kernels on gfx950; there is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, Mapping, Sequence

import numpy as np

from . import _native as _NATIVE_MODULE

# The seam the reference's tests monkeypatch (tests/test_hybrid_terrain_pt.py:860-876).
_NATIVE = _NATIVE_MODULE

_TEXTUAL = (str, bytes, bytearray, memoryview)


# ---- sun colour ------------------------------------------------------------------------------------
def _three_floats(value) -> tuple:
    """Length and float conversion of a colour triple; raises the TypeError / ValueError Python itself
    produces (their text is part of the contract: 'object of type 'float' has no len()')."""
    count = len(value)
    if count != 3:
        raise ValueError(f"sun_color must have exactly three components, got {count}")
    return tuple(map(float, (value[0], value[1], value[2])))


def _parse_sun_color(value) -> tuple:
    if isinstance(value, _TEXTUAL):
        raise ValueError(f"sun_color must be three numbers, got {value!r}")
    try:
        rgb = _three_floats(value)
    except (TypeError, ValueError) as problem:
        raise ValueError(f"sun_color must be a sequence of three numbers: {problem}")
    for test, what in ((lambda raw, c: isinstance(raw, _TEXTUAL), "numbers"),
                       (lambda raw, c: not np.isfinite(c), "finite"),
                       (lambda raw, c: c < 0.0, "non-negative")):
        if any(test(raw, c) for raw, c in zip(value, rgb)):
            raise ValueError(f"sun_color components must be {what}, got {value!r}")
    return rgb


# ---- the normalised call ---------------------------------------------------------------------------
@dataclass
class _Request:
    dem: np.ndarray
    width: int
    height: int
    camera: dict
    opt: dict                      # keyword options by name, as passed
    env: "np.ndarray | None" = None
    mesh_v: "np.ndarray | None" = None
    mesh_i: "np.ndarray | None" = None
    sun_rgb: tuple = field(default=(1.0, 0.97, 0.92))


# Ordered rejection rules: (is the request bad?, message).  Evaluated top to bottom, first hit raises.
_RULES: "tuple[tuple[Callable[[_Request], bool], Callable[[_Request], str]], ...]" = (
    (lambda q: q.dem.ndim != 2,
     lambda q: f"heightmap must be 2D (H, W), got shape {q.dem.shape}"),
    (lambda q: min(q.dem.shape) < 2,
     lambda q: f"terrain heightfield must be at least 2x2 texels, got {q.dem.shape[1]}x{q.dem.shape[0]}"),
    # (min / max propagate NaN and keep infinities: two reductions instead of a 4 MB temporary -- 0.9 instead of 3.6 ms for a 2048^2 DEM)
    (lambda q: not (np.isfinite(q.dem.min()) and np.isfinite(q.dem.max())),
     lambda q: "heightmap contains non-finite samples"),
    (lambda q: int(q.opt["min_frames"]) > int(q.opt["max_frames"]),
     lambda q: f"min_frames ({q.opt['min_frames']}) must be <= max_frames ({q.opt['max_frames']})"),
    (lambda q: not 1 <= int(q.opt["spp"]) <= 64,
     lambda q: f"spp must be in 1..=64, got {q.opt['spp']}"),
    (lambda q: not all(float(s) > 0.0 for s in q.opt["spacing"][:2]),
     lambda q: f"spacing must be > 0, got {q.opt['spacing']}"),
)


def _coerce_scene_arrays(q: _Request) -> None:
    """Environment map and mesh: shapes checked after the sun has been resolved, like the reference."""
    env_map, verts, faces = q.opt["env_map"], q.opt["mesh_vertices"], q.opt["mesh_indices"]
    if env_map is not None:
        q.env = np.ascontiguousarray(env_map, dtype=np.float32)
        if q.env.ndim != 3 or q.env.shape[2] != 3:
            raise ValueError(f"env_map must be (H, W, 3) float32, got {q.env.shape}")
    if (verts is None) is not (faces is None):
        raise ValueError("mesh_vertices and mesh_indices must be provided together")
    if verts is None:
        return
    q.mesh_v = np.ascontiguousarray(verts, dtype=np.float32)
    q.mesh_i = np.ascontiguousarray(faces, dtype=np.uint32)
    for arr, label, letter in ((q.mesh_v, "mesh_vertices", "N"), (q.mesh_i, "mesh_indices", "M")):
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise ValueError(f"{label} must be ({letter}, 3), got {arr.shape}")


# ---- where the sun comes from ----------------------------------------------------------------------
_MANUAL_SUN_DEFAULTS = {"sun_azimuth_deg": 315.0, "sun_elevation_deg": 45.0, "observer_latitude_deg": 0.0,
                        "observer_longitude_deg": 0.0, "pressure_mbar": 1013.25, "temperature_c": 15.0}


@dataclass
class _SunResolution:
    source: str
    values: dict  # the six keys of _MANUAL_SUN_DEFAULTS, resolved

    @classmethod
    def of(cls, opt: Mapping[str, Any]) -> "_SunResolution":
        given = {name: opt[name] for name in _MANUAL_SUN_DEFAULTS}
        when = opt["solar_time"]
        if when is None:
            return cls("manual_angles", {name: (default if given[name] is None else given[name])
                                         for name, default in _MANUAL_SUN_DEFAULTS.items()})
        if not all(v is None for v in given.values()):
            raise ValueError(
                "solar_time cannot be combined with manual sun, observer, pressure, or temperature values")
        # The reference evaluates SolarTime with its native NREL SPA (python/forge3d/geo.py:23-52,
        # src/geo/solar.rs:77); here forge3d_amd.geo does (adjacent to the hot path).
        from .geo import resolve_solar_time

        solar = resolve_solar_time(when)
        elevation = "true_elevation_deg" if opt["refraction_model"] == "none" else "apparent_elevation_deg"
        return cls("solar_time", {
            "sun_azimuth_deg": solar["azimuth_deg"], "sun_elevation_deg": solar[elevation],
            "observer_latitude_deg": solar["observer_lat"], "observer_longitude_deg": solar["observer_lon"],
            "pressure_mbar": solar["pressure_mbar"], "temperature_c": solar["temperature_c"]})


# ---- what the native function receives --------------------------------------------------------------
def _floats(n: int) -> Callable[[Any], tuple]:
    return lambda v: tuple(float(v[i]) for i in range(n))


def _as_is(v):
    return v


# keyword -> conversion, in the native function's order (src/py_functions/path_tracing/terrain_reference.rs:224-256)
_NATIVE_KEYWORDS: "tuple[tuple[str, Callable[[Any], Any]], ...]" = (
    ("spacing", _floats(2)), ("exaggeration", float), ("albedo", _floats(3)), ("sun_azimuth_deg", float),
    ("sun_elevation_deg", float), ("sun_intensity", float), ("sun_color", _as_is), ("env_map", _as_is),
    ("env_intensity", float), ("mesh_vertices", _as_is), ("mesh_indices", _as_is), ("spp", int),
    ("max_frames", int), ("min_frames", int), ("variance_threshold", float), ("seed", int),
    ("certificate", _as_is), ("observer_latitude_deg", float), ("observer_longitude_deg", float),
    ("earth_model", _as_is), ("sphere_radius_m", float), ("refraction_model", _as_is), ("refraction_k", float),
    ("pressure_mbar", float), ("temperature_c", float), ("atmosphere", _as_is),
)


def hybrid_render_terrain_reference(
        heightmap: "np.ndarray", width: int, height: int, camera: "dict | None" = None, *,
        spacing: "tuple[float, float]" = (1.0, 1.0), exaggeration: float = 1.0,
        albedo: "tuple[float, float, float]" = (0.6, 0.6, 0.6),
        sun_azimuth_deg: float | None = None, sun_elevation_deg: float | None = None,
        solar_time: "object | None" = None, sun_intensity: float = 2.5,
        sun_color: "Sequence[float] | np.ndarray" = (1.0, 0.97, 0.92),
        env_map: "np.ndarray | None" = None, env_intensity: float = 0.35,
        mesh_vertices: "np.ndarray | None" = None, mesh_indices: "np.ndarray | None" = None,
        spp: int = 1, max_frames: int = 512, min_frames: int = 32, variance_threshold: float = 1e-3, seed: int = 7,
        certificate: bool | str = False, cache: str | None = None,
        observer_latitude_deg: float | None = None, observer_longitude_deg: float | None = None,
        earth_model: str = "ellipsoid", sphere_radius_m: float = 6_371_008.8,
        refraction_model: str = "bennett", refraction_k: float = 0.13,
        pressure_mbar: float | None = None, temperature_c: float | None = None,
        atmosphere: "Mapping[str, Any] | Any | None" = None,
) -> dict:
    """Converged path-traced reference image of a DEM under sun + sky on an MI355X.

    Accumulates frames of ``spp`` tent-jittered camera samples (heightfield traversal with the exact
    bilinear-patch solve, the sun through the ReSTIR reservoir chain, one cosine-weighted sky ray) until the
    per-pixel variance of the running-mean luminance over the last 32-frame window is below
    ``variance_threshold``; an unconverged render raises, it never returns.  Result: ``rgba`` (H,W,4) uint8,
    ``albedo`` / ``normal`` (H,W,3) float32, ``depth`` (H,W) float32 with NaN where nothing was hit,
    ``frames``, ``variance``, ``converged``, the memory diagnostics, and ``sun_source`` /
    ``solar_azimuth_deg`` / ``solar_elevation_deg``.  ``cache`` is accepted and ignored.
    """
    options = dict(locals())
    for positional in ("heightmap", "width", "height", "camera"):
        options.pop(positional)
    if getattr(_NATIVE, "hybrid_render_terrain_reference", None) is None:
        raise RuntimeError("hybrid_render_terrain_reference requires the native forge3d module with GPU support")

    request, sun, keywords = _prepare(heightmap, width, height, camera, options)
    result = _NATIVE.hybrid_render_terrain_reference(request.dem, request.width, request.height, request.camera,
                                                     **keywords)
    return _with_sun(result, sun)


def _prepare(heightmap, width, height, camera, options: dict):
    """The wrapper's checks, in its order, and the native keyword set of one call: (request, sun, keywords)."""
    request = _Request(np.ascontiguousarray(heightmap, dtype=np.float32), int(width), int(height),
                       dict(camera or {}), options)
    for is_bad, message in _RULES:
        if is_bad(request):
            raise ValueError(message(request))
    request.sun_rgb = _parse_sun_color(options["sun_color"])
    sun = _SunResolution.of(options)
    _coerce_scene_arrays(request)

    values = {**options, **sun.values, "sun_color": request.sun_rgb, "env_map": request.env,
              "mesh_vertices": request.mesh_v, "mesh_indices": request.mesh_i}
    keywords = {name: convert(values[name]) for name, convert in _NATIVE_KEYWORDS}
    return request, sun, keywords


def _with_sun(result: dict, sun: _SunResolution) -> dict:
    result.update(sun_source=sun.source, solar_azimuth_deg=float(sun.values["sun_azimuth_deg"]),
                  solar_elevation_deg=float(sun.values["sun_elevation_deg"]))
    return result


# ---- a sequence of renders of one scene under changing suns: one live session, re-armed per frame ----------------------
# per-frame keys a live session can change (forge3d_amd.session.TerrainSession.rearm); solar_time resolves to some of them
SEQUENCE_FRAME_KEYS = ("sun_azimuth_deg", "sun_elevation_deg", "solar_time", "sun_intensity", "sun_color", "env_intensity",
                       "seed", "max_frames", "min_frames", "variance_threshold", "observer_latitude_deg",
                       "observer_longitude_deg", "pressure_mbar", "temperature_c")


def render_terrain_sequence(heightmap: "np.ndarray", width: int, height: int, camera: "dict | None" = None, *,
                            frames: "Sequence[Mapping[str, Any]]", **common):
    """Generator: item i equals ``hybrid_render_terrain_reference(heightmap, width, height, camera, **common, **frames[i])``.

    ``common`` takes the wrapper's keywords; ``frames[i]`` only keys a live session can change (SEQUENCE_FRAME_KEYS: the
    sun by angles or ``solar_time``, intensity, colour, IBL intensity, seed, frame budget, observer / air for the
    refraction).  Every frame is checked by the wrapper's own rules before any device work; then ONE session renders the
    whole sequence, re-armed between frames (f3d_session_rearm: no new tables, allocations or G-buffer pass).
    """
    yield from _render_sequence("render_terrain_sequence", heightmap, width, height, camera, frames, common)


def render_terrain_camera_sequence(heightmap: "np.ndarray", width: int, height: int, *,
                                   frames: "Sequence[Mapping[str, Any]]", **common):
    """Generator: item i equals ``hybrid_render_terrain_reference(heightmap, width, height, frames[i]["camera"], **common,
    **rest_of_frames[i])`` -- an orbit or a fly-over of one DEM.

    ``frames[i]`` must hold ``"camera"`` (a camera dict, read as the one-shot call reads it: missing keys take the
    wrapper's defaults) and may hold any of SEQUENCE_FRAME_KEYS.  Every frame is checked by the wrapper's own rules
    before any device work; then ONE session renders the whole sequence, re-aimed between frames (f3d_session_reaim: no
    new tables, allocations, streams or clears -- one pass traces the centre rays of the new view).
    """
    yield from _render_sequence("render_terrain_camera_sequence", heightmap, width, height, None, frames, common)


def render_terrain_mesh_sequence(heightmap: "np.ndarray", width: int, height: int, camera: "dict | None" = None, *,
                                 frames: "Sequence[Mapping[str, Any]]", **common):
    """Generator: item i equals ``hybrid_render_terrain_reference(heightmap, width, height, camera_i, **common,
    **frames[i])`` -- geometry moving on one DEM (a vehicle, turbine blades, buildings growing).

    ``common`` must hold a mesh (``mesh_vertices`` and ``mesh_indices``).  ``frames[i]`` may hold ``"mesh_vertices"``
    (on the indices of ``common``: the session's BVH is refitted on the GPU), optionally ``"mesh_indices"`` (another
    mesh: built as a new session builds it), optionally ``"camera"`` (camera_i; without it the positional ``camera``) and
    any of SEQUENCE_FRAME_KEYS; a key a frame does not name is ``common``'s, as in the one-shot call.  Every frame is
    checked by the wrapper's own rules before any device work; then ONE session renders the whole sequence, re-meshed
    between frames (f3d_session_remesh) wherever the mesh changes.
    """
    if common.get("mesh_vertices") is None or common.get("mesh_indices") is None:
        raise ValueError("render_terrain_mesh_sequence needs the mesh in the common keywords (mesh_vertices and mesh_indices): a "
                         "live session cannot be given a mesh it was created without")
    yield from _render_sequence("render_terrain_mesh_sequence", heightmap, width, height, camera, frames, common)


def render_terrain_dem_sequence(heightmap: "np.ndarray", width: int, height: int, camera: "dict | None" = None, *,
                                frames: "Sequence[Mapping[str, Any]]", **common):
    """Generator: item i equals ``hybrid_render_terrain_reference(frames[i]["heightmap"], width, height, camera_i, **common,
    **rest_of_frames[i])`` -- ground that moves: a glacier, lava or flood time-lapse, an erosion or excavation run, a
    sweep of the exaggeration.

    ``frames[i]`` may hold ``"heightmap"`` (a DEM of the positional one's shape; without it the positional ``heightmap``),
    optionally ``"exaggeration"`` (without it ``common``'s), optionally ``"camera"`` (camera_i; without it the positional
    ``camera``) and any of SEQUENCE_FRAME_KEYS.  Every frame is checked by the wrapper's own rules before any device work,
    and a frame whose DEM has another shape is refused (another DEM size needs a new session); then ONE session renders the
    whole sequence, re-terrained between frames (f3d_session_reterrain: the samples uploaded in stream order, the
    session's tables patched on the GPU) wherever the DEM or the exaggeration changes.
    """
    yield from _render_sequence("render_terrain_dem_sequence", heightmap, width, height, camera, frames, common)


# generator -> (a frame must / may / may not hold "camera", its keys beyond SEQUENCE_FRAME_KEYS, the strongest update the generator
# admits: a frame that does not need it falls through to a re-aim -- under "rearm", which has no per-frame camera, to a re-arm)
_SEQUENCES = {
    "render_terrain_sequence": ("may not", (), "rearm"),
    "render_terrain_camera_sequence": ("must", (), "reaim"),
    "render_terrain_mesh_sequence": ("may", ("mesh_vertices", "mesh_indices"), "remesh"),
    "render_terrain_dem_sequence": ("may", ("heightmap", "exaggeration"), "reterrain"),
}


def _render_sequence(name, heightmap, width, height, camera, frames, common):
    """The sequence generators: one session, updated between frames as _SEQUENCES[name] says."""
    import inspect

    from .session import TerrainSession

    frame_camera, extra_keys, update = _SEQUENCES[name]
    signature = inspect.signature(hybrid_render_terrain_reference)
    defaults = {key: p.default for key, p in signature.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    for key in common:
        if key not in defaults:
            raise TypeError(f"{name}() got an unexpected keyword argument {key!r}")
    frames = [dict(f) for f in frames]
    cameras = []
    for i, frame in enumerate(frames):
        if frame_camera == "must" and "camera" not in frame:
            raise ValueError(f"frames[{i}] lacks 'camera': every frame of {name} names its camera (a sequence under "
                             "one camera is render_terrain_sequence's)")
        cameras.append(frame.pop("camera") if frame_camera != "may not" and "camera" in frame else camera)
        for key in frame:
            if key not in extra_keys and key not in SEQUENCE_FRAME_KEYS:
                raise ValueError(f"frames[{i}] sets {key!r}, which a live session cannot change (per-frame keys: "
                                 f"{', '.join(SEQUENCE_FRAME_KEYS)}); render it with hybrid_render_terrain_reference")
    if getattr(_NATIVE, "hybrid_render_terrain_reference", None) is None:
        raise RuntimeError("hybrid_render_terrain_reference requires the native forge3d module with GPU support")
    dems = [frame.pop("heightmap", heightmap) if "heightmap" in extra_keys else heightmap for frame in frames]
    calls = [_prepare(dem, width, height, cam, {**defaults, **common, **frame}) for dem, cam, frame in zip(dems, cameras, frames)]
    if not calls:
        return
    for i, (request, _, _) in enumerate(calls):
        if request.dem.shape != calls[0][0].dem.shape:
            raise ValueError(f"frames[{i}] has a heightmap of shape {request.dem.shape}, the sequence's DEM has {calls[0][0].dem.shape}: "
                             "a live session keeps its DEM size (render it with hybrid_render_terrain_reference)")
    request, _, first = calls[0]
    native = dict(first)
    native.pop("certificate")
    native["atmosphere"] = _NATIVE_MODULE._resolve_atmosphere(native["atmosphere"])
    # one-shot calls size frames in flight automatically: so does the session (same byte counts in the result)
    session = TerrainSession(request.dem, request.width, request.height, request.camera,
                             frames_in_flight=_NATIVE_MODULE.FRAMES_IN_FLIGHT_AUTO, **native)
    held = (first["mesh_vertices"], first["mesh_indices"])  # the mesh the session holds
    held_dem = (request.dem, first["exaggeration"])  # the DEM and exaggeration the session holds
    try:
        for i, (request, sun, keywords) in enumerate(calls):
            if i:
                values = {key: keywords[key] for key in TerrainSession.REARMABLE if key in keywords}
                mesh = (keywords["mesh_vertices"], keywords["mesh_indices"])
                dem = (request.dem, keywords["exaggeration"])
                # which update frame i needs: the DEM (by bits: -0.0 is another DEM) or the exaggeration differs: a re-terrain;
                # else the mesh differs: a re-mesh (equal indices: a refit on the topology the session holds, else the create's
                # path); else a re-aim, or without per-frame cameras a re-arm
                if update == "reterrain" and not (dem[1] == held_dem[1] and np.array_equal(dem[0].view(np.uint32), held_dem[0].view(np.uint32))):
                    session.reterrain(dem[0], request.camera, exaggeration=dem[1], **values)
                    held_dem = dem
                elif update == "remesh" and not (np.array_equal(mesh[0], held[0]) and np.array_equal(mesh[1], held[1])):
                    session.remesh(mesh[0], None if np.array_equal(mesh[1], held[1]) else mesh[1], request.camera, **values)
                    held = mesh
                elif update == "rearm":
                    session.rearm(**values)
                else:
                    session.reaim(request.camera, **values)
            yield _with_sun(session.render(), sun)
    finally:
        session.close()
