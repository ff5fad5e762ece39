"""``ViewerHandle`` / ``open_viewer`` / ``Renderer`` names of the reference, routed to the terrain path tracer.

forge3d's ``ViewerHandle`` (reference python/forge3d/viewer.py:181-1383) remote-controls an interactive RASTER
viewer process over IPC and ``Renderer`` (python/forge3d/__init__.py:347-421) is a CPU triangle stub; neither is
path traced, so no golden of the reference can pin what ``snapshot()`` draws here -- parity for this facade is
UNPINNED.  What carries over is the calling surface a script written against forge3d uses for an
offline render: ``open_viewer_async(width, height, terrain_path=..., fov_deg=...)`` -> ``ViewerHandle`` with
``load_terrain``, ``set_orbit_camera``, ``set_camera_lookat``, ``set_fov``, ``set_sun``, ``set_sun_time``, ``set_ibl``,
``set_z_scale``, ``snapshot(path, width, height)``, ``render_animation``, ``get_stats``, ``close`` and the context
manager.  There is no subprocess and no window: every snapshot is a converged path-traced frame on the MI355X.
``load_overlay`` drapes ONE image over the terrain as its per-texel albedo (TerrainSession.drape) and ``add_vector_overlay``
paints points, lines and triangles into that drape on the GPU (TerrainSession.paint).  Commands of the raster viewer that
have no meaning offline (labels, point clouds) raise ``ViewerError`` instead of being ignored.
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import io as _io
from .offline import OfflineTerrainViewer


class ViewerError(Exception):
    """reference python/forge3d/viewer.py:160-162"""


_RASTER_ONLY = ("load_obj", "load_gltf", "load_bundle", "load_point_cloud", "set_point_cloud_params",
                "set_transform", "add_label", "add_labels", "add_line_label", "add_curved_label", "add_callout",
                "set_labels_enabled", "clear_labels", "remove_label", "set_label_typography",
                "set_declutter_algorithm", "poll_pick_events", "update_labels", "load_label_atlas",
                "set_terrain_scatter", "clear_terrain_scatter", "apply_scene_variant", "set_review_layer_visible")


class ViewerHandle(OfflineTerrainViewer):
    """Offline stand-in for the reference's ViewerHandle: same method names and argument order."""

    def __init__(self, width: int = 1280, height: int = 720, *, fov_deg: float = 60.0, spp: int = 8, **render):
        super().__init__(width, height, spp=spp, **render)
        self._fov = float(fov_deg)
        self._env = None
        self._env_intensity = 0.35
        self._sun_intensity = 2.5
        self._revision = 0
        self._open = True
        self._overlay = None
        self._vector_layers = {}
        self._contours = None
        self._streams = None
        self._vector_next_id = 1
        self._vector_canvas = None

    # -- scene --------------------------------------------------------------------------------------------
    def load_terrain(self, path: Union[str, Path, np.ndarray], spacing: Union[float, Tuple[float, float], None] = None) -> None:
        """reference viewer.py:978-986 takes a DEM path; arrays are accepted too.  Spacing defaults to the
        GeoTIFF pixel scale when the file carries one, else 1."""
        if spacing is None and not isinstance(path, np.ndarray) and str(path).lower().endswith((".tif", ".tiff")):
            scale = _io.read_geotiff(path)[1]["pixel_scale"]
            spacing = (float(scale[0]), float(scale[1])) if scale else 1.0
        super().load_terrain(path, 1.0 if spacing is None else spacing)
        self._revision += 1

    def set_sun(self, azimuth_deg: float, elevation_deg: float) -> None:
        super().set_sun(azimuth_deg, elevation_deg)
        self._revision += 1

    def set_sun_time(self, solar_time: Any, intensity: float = 1.0) -> None:
        """reference viewer.py:1128-1145: the apparent position of a forge3d.geo.SolarTime-like object."""
        from .geo import resolve_solar_time

        position = resolve_solar_time(solar_time)
        super().set_sun(float(position["azimuth_deg"]), float(position["apparent_elevation_deg"]))
        self._sun_intensity = 2.5 * float(intensity)
        self._revision += 1

    def set_ibl(self, path: Union[str, Path, np.ndarray], intensity: float = 1.0) -> None:
        """Environment map: a Radiance .hdr / .rgbe file (reference viewer.py:1147, loader src/formats/hdr.rs), an
        (H, W, 3) float32 array, or a .npy file of one."""
        if isinstance(path, np.ndarray):
            env = path
        elif Path(path).suffix.lower() in (".hdr", ".rgbe"):
            try:
                env = _io.read_hdr(path)
            except (OSError, _io.HdrError) as exc:
                raise ViewerError(str(exc)) from exc
        elif Path(path).suffix.lower() == ".npy":
            env = np.load(Path(path))
        else:
            raise ViewerError(f"Unsupported environment map format '{Path(path).suffix}' for '{path}': expected .hdr, .rgbe or .npy")
        env = np.ascontiguousarray(env, np.float32)
        if env.ndim != 3 or env.shape[2] != 3:
            raise ViewerError(f"environment map must be (H, W, 3) float32, got {env.shape}")
        self._env, self._env_intensity = env, float(intensity)
        self._revision += 1

    def load_overlay(self, name: str, path: Union[str, Path, np.ndarray], extent: Optional[Sequence[float]] = None,
                     opacity: Optional[float] = None, z_order: Optional[int] = None, preserve_colors: Optional[bool] = None, *,
                     filter: str = "bilinear", srgb: Optional[bool] = None) -> None:
        """reference viewer.py:1009-1042, as far as a path tracer has a counterpart: the image becomes the terrain's albedo
        (the viewer keeps no session between renders: every later render() / snapshot() creates its session, drapes it with
        this image through TerrainSession.drape and renders; render_animation() drapes ONE session and re-aims it per key), lit
        and shadowed like the ground it lies on.  ``path``: an 8-bit PNG (read by forge3d_amd.io), a .npy file, or an ``(H, W, 3|4)`` array -- uint8 or
        float32; row 0 lies on DEM row 0.  ``extent`` is the reference's normalised ``(u0, v0, u1, v1)`` of the DEM's footprint
        the image covers (u along DEM columns, v along DEM rows; default the whole DEM); outside it the image's edge texels
        continue (clamp to edge).  ``srgb``: decode to linear first (default: yes for files and uint8 arrays, no for float32).
        ONE overlay at a time: loading another replaces it whatever its name.  ``opacity``, ``z_order`` and
        ``preserve_colors`` belong to the raster viewer's compositor and are refused when given."""
        for key, value in (("opacity", opacity), ("z_order", z_order), ("preserve_colors", preserve_colors)):
            if value is not None:
                raise ViewerError(f"ViewerHandle.load_overlay({key}=...) belongs to the interactive raster viewer's compositor; the "
                                  "offline path tracer drapes the image as the terrain's albedo and has no counterpart")
        if filter not in ("nearest", "bilinear"):
            raise ViewerError(f"overlay filter must be 'nearest' or 'bilinear', got {filter!r}")
        if isinstance(path, np.ndarray):
            image, from_file = path, False
        elif Path(path).suffix.lower() == ".png":
            try:
                image, from_file = _io.png_to_numpy(path), True
            except (OSError, ValueError) as exc:
                raise ViewerError(str(exc)) from exc
        elif Path(path).suffix.lower() == ".npy":
            image, from_file = np.load(Path(path)), True
        else:
            raise ViewerError(f"Unsupported overlay format '{Path(path).suffix}' for '{path}': expected .png or .npy")
        if image.ndim == 2:
            image = np.repeat(image[:, :, None], 3, 2)
        elif image.ndim == 3 and image.shape[2] == 2:  # grey + alpha
            image = np.repeat(image[:, :, :1], 3, 2)
        if image.ndim != 3 or image.shape[2] not in (3, 4) or image.dtype not in (np.uint8, np.float32):
            raise ViewerError(f"overlay must be (H, W, 3|4) uint8 or float32, got {image.dtype} {image.shape}")
        if extent is None:
            extent = (0.0, 0.0, 1.0, 1.0)
        u0, v0, u1, v1 = (float(v) for v in extent)
        if not (np.isfinite([u0, v0, u1, v1]).all() and u1 > u0 and v1 > v0):
            raise ViewerError(f"overlay extent must be finite (u0, v0, u1, v1) with u1 > u0 and v1 > v0, got {tuple(extent)}")
        decode = (from_file or image.dtype == np.uint8) if srgb is None else bool(srgb)
        self._overlay = {"name": str(name), "image": np.ascontiguousarray(image), "extent": (u0, v0, u1, v1), "filter": filter,
                         "srgb": decode}
        self._revision += 1

    def remove_overlay(self, name: str) -> None:
        """Take the overlay ``name`` off again (reference viewer.py remove_overlay)."""
        if getattr(self, "_overlay", None) is None or self._overlay["name"] != str(name):
            raise ViewerError(f"no overlay named {name!r}")
        self._overlay = None
        self._revision += 1

    @staticmethod
    def overlay_registration(dem_shape, image_shape, extent):
        """(scale_x, offset_x, scale_z, offset_z) of TerrainSession.drape for an image that covers the normalised extent
        (u0, v0, u1, v1) of the DEM edge to edge: t = ((f / (n - 1)) - u0) / (u1 - u0) * texels - 0.5."""
        (dem_h, dem_w), (rows, cols), (u0, v0, u1, v1) = dem_shape, image_shape[:2], extent
        return (cols / ((dem_w - 1) * (u1 - u0)), -u0 * cols / (u1 - u0) - 0.5,
                rows / ((dem_h - 1) * (v1 - v0)), -v0 * rows / (v1 - v0) - 0.5)

    # -- vector overlays: painted into the drape (TerrainSession.paint) ------------------------------------------------
    VECTOR_PRIMITIVES = ("points", "lines", "line_strip", "triangles", "triangle_strip")
    VECTOR_CANVAS_TEXELS_PER_CELL, VECTOR_CANVAS_MAX_SIDE = 4, 8192

    # what a row of add_vector_overlay can be refused for, in the order a row is looked at; the texts are the reference's
    # (recorded in tests/golden/vector_overlay_messages.json)
    VECTOR_VERTEX_REFUSALS = ("must contain exactly 8 lanes: XYZ, RGBA, feature ID", "XYZ must be finite f64",
                              "RGBA must be finite values in [0, 1]", "feature ID must be an integer u32")

    @staticmethod
    def feature_id(value) -> Optional[int]:
        """The feature id a vertex row's last lane stands for, or None when it is not a whole number in [0, 2^32) -- a bool, text
        that is no number, None, a fraction, NaN, an infinity."""
        if value is True or value is False:
            return None
        try:
            number = float(value)
        except (TypeError, ValueError):
            return None
        if not 0.0 <= number < 2.0 ** 32:  # (NaN compares false)
            return None
        whole = int(number)
        return whole if whole == number else None

    @classmethod
    def vector_overlay_vertices(cls, vertices) -> np.ndarray:
        """The rows of ``add_vector_overlay`` as an ``(N, 8)`` float64 array: eight lanes a row (X, Y, Z, R, G, B, A, feature
        id), finite XYZ, RGBA in [0, 1], the id a whole number in [0, 2^32).  The first row that is not, and the first thing
        wrong with it in that order, is refused with the reference's message for it."""
        rows = list(vertices)
        n = len(rows)
        whole = np.array([len(row) == 8 for row in rows], bool).reshape(n)
        ids = [cls.feature_id(row[7]) if ok else None for row, ok in zip(rows, whole)]
        table = np.zeros((n, 8), np.float64)
        if whole.any():
            table[whole, :7] = np.array([list(row[:7]) for row, ok in zip(rows, whole) if ok], np.float64)
        table[:, 7] = [0.0 if i is None else float(i) for i in ids]
        rgba = table[:, 3:7]
        with np.errstate(invalid="ignore"):
            wrong = np.stack([~whole, ~np.isfinite(table[:, :3]).all(1), ~((rgba >= 0.0) & (rgba <= 1.0)).all(1),  # (NaN compares false)
                              np.array([i is None for i in ids], bool).reshape(n)], 1)
        bad_rows = np.flatnonzero(wrong.any(1))
        if bad_rows.size:
            row = int(bad_rows[0])
            raise ValueError(f"vector vertex {row} {cls.VECTOR_VERTEX_REFUSALS[int(np.argmax(wrong[row]))]}")
        return table

    @staticmethod
    def expand_strip(indices, primitive: str):
        """(list primitive, index list) of ``primitive`` over ``indices``: ``line_strip`` becomes the segments (i, i + 1),
        ``triangle_strip`` the triangles (i, i + 1, i + 2) with every second one's first two swapped (one winding); the list
        kinds pass through."""
        idx = np.asarray(indices, np.int64).ravel()
        if primitive == "line_strip":
            return "lines", np.stack([idx[:-1], idx[1:]], 1).ravel() if idx.size >= 2 else idx[:0]
        if primitive == "triangle_strip":
            if idx.size < 3:
                return "triangles", idx[:0]
            tri = np.stack([idx[:-2], idx[1:-1], idx[2:]], 1)
            tri[1::2, :2] = tri[1::2, 1::-1]
            return "triangles", tri.ravel()
        return primitive, idx

    def add_vector_overlay(self, name: str, vertices, indices, primitive: str = "triangles", drape: bool = True,
                           drape_offset: float = 0.5, opacity: float = 1.0, depth_bias: float = 0.001, line_width: float = 2.0,
                           point_size: float = 5.0, z_order: int = 0) -> int:
        """reference viewer.py add_vector_overlay, as far as an offline path tracer has a counterpart: the layer is painted into
        the terrain's drape on the GPU (TerrainSession.paint) by every later render() / snapshot() / render_animation(), lit
        and shadowed like the ground it lies on.  ``vertices``: the reference's eight-lane rows (X, Y, Z, R, G, B, A, feature
        id); under ``drape=True`` Y is ignored and X, Z are world x, z of the terrain (its centre is the origin).
        ``drape=False`` -- an undraped 3-D overlay -- has no offline counterpart and raises.  ``primitive``: ``"points"``,
        ``"lines"``, ``"line_strip"``, ``"triangles"`` or ``"triangle_strip"`` (strips are expanded to lists here).
        ``line_width`` and ``point_size`` are in CANVAS TEXELS (the reference's are screen pixels, which an offline render of
        any size and camera does not have); the canvas is the loaded overlay image, or else a constant image of the terrain's
        albedo with four texels per DEM cell and axis (at most 8192 a side; set_vector_canvas overrides).  ``drape_offset`` and
        ``depth_bias`` steer the raster viewer's depth test and are accepted and ignored.  Layers are painted in
        ``(z_order, id)`` order.  Returns the layer's id."""
        if not drape:
            raise ViewerError("ViewerHandle.add_vector_overlay(drape=False) is an undraped 3-D overlay of the interactive raster viewer; "
                              "the offline path tracer paints vector overlays into the terrain's drape only")
        if primitive not in self.VECTOR_PRIMITIVES:
            raise ViewerError(f"vector overlay primitive must be one of {', '.join(self.VECTOR_PRIMITIVES)}, got {primitive!r}")
        rows = self.vector_overlay_vertices(vertices)
        if rows.shape[0] == 0:
            raise ViewerError("a vector overlay needs at least one vertex")
        raw = [int(i) for i in indices]
        if any(i < 0 or i >= rows.shape[0] for i in raw):
            raise ViewerError(f"vector overlay indices must lie in [0, {rows.shape[0]})")
        kind, idx = self.expand_strip(raw, str(primitive))
        per = {"points": 1, "lines": 2, "triangles": 3}[kind]
        if idx.size == 0 or idx.size % per:
            raise ViewerError(f"{len(raw)} indices do not make {primitive}")
        opacity, line_width, point_size = float(opacity), float(line_width), float(point_size)
        if not 0.0 <= opacity <= 1.0:
            raise ViewerError(f"vector overlay opacity must lie in [0, 1], got {opacity}")
        if not (np.isfinite([line_width, point_size]).all() and line_width >= 0.0 and point_size >= 0.0):
            raise ViewerError("vector overlay line_width and point_size must be finite and >= 0 canvas texels")
        _ = drape_offset, depth_bias
        layer_id = self._vector_next_id
        self._vector_next_id = layer_id + 1
        self._vector_layers[layer_id] = {"name": str(name), "xz": rows[:, [0, 2]].astype(np.float32), "rgba": rows[:, 3:7].astype(np.float32),
                            "features": rows[:, 7].astype(np.uint32), "primitive": kind, "indices": idx.astype(np.uint32),
                            "texels": point_size if kind == "points" else line_width, "opacity": opacity, "z_order": int(z_order)}
        self._revision += 1
        return layer_id

    def remove_vector_overlay(self, overlay_id: int) -> None:
        """Take the layer ``overlay_id`` (what add_vector_overlay returned) off again."""
        if int(overlay_id) not in self._vector_layers:
            raise ViewerError(f"no vector overlay with id {overlay_id}")
        del self._vector_layers[int(overlay_id)]
        self._revision += 1

    def set_vector_canvas(self, rows: Optional[int], cols: Optional[int] = None) -> None:
        """The size of the constant canvas vector overlays are painted into when no overlay image is loaded (``None``: the
        default, four texels per DEM cell and axis, at most 8192 a side)."""
        if rows is None:
            self._vector_canvas = None
        else:
            rows, cols = int(rows), int(rows if cols is None else cols)
            if not (1 <= rows <= 16384 and 1 <= cols <= 16384):
                raise ViewerError(f"the vector canvas holds 1..16384 texels a side, got {rows} x {cols}")
            self._vector_canvas = (rows, cols)
        self._revision += 1

    def vector_layers(self) -> list:
        """The layers in the order they are painted: by ``(z_order, id)``."""
        layers = self._vector_layers
        return [layers[i] for i in sorted(layers, key=lambda i: (layers[i]["z_order"], i))]

    def vector_canvas_shape(self, dem_shape) -> Tuple[int, int]:
        if self._vector_canvas is not None:
            return self._vector_canvas
        k, cap = self.VECTOR_CANVAS_TEXELS_PER_CELL, self.VECTOR_CANVAS_MAX_SIDE
        return (min(k * max(dem_shape[0] - 1, 1), cap), min(k * max(dem_shape[1] - 1, 1), cap))

    def enable_contours(self, interval: float, *, base: float = 0.0, width: float = 1.5, rgba=(0.0, 0.0, 0.0, 0.8), index_every: int = 0,
                        index_width: float = 3.0) -> None:
        """Contour lines of the terrain as it is rendered (heights times the z scale), every ``interval`` from ``base``, painted
        on the GPU from the session's own tables (TerrainSession.paint_contours) after the overlay image and before the vector
        layers.  ``width`` and ``index_width`` are stroke widths in canvas texels, like a vector layer's ``line_width``;
        ``index_every`` = n > 0 paints every n-th level (counted from ``base``) a second time ``index_width`` wide.  ``rgba``:
        linear colour and alpha, default the reference overlay's."""
        interval, base, width, index_width = float(interval), float(base), float(width), float(index_width)
        if not np.isfinite(interval) or interval <= 0.0 or not np.isfinite(base):
            raise ViewerError(f"contour interval must be finite and > 0 and base finite, got interval={interval}, base={base}")
        if not (np.isfinite(width) and width >= 0.0 and np.isfinite(index_width) and index_width >= 0.0):
            raise ViewerError(f"contour widths must be finite and >= 0 texels, got {width} and {index_width}")
        colour = np.asarray(rgba, np.float32).reshape(-1)
        if colour.shape[0] not in (3, 4) or not np.all((colour >= 0.0) & (colour <= 1.0)):
            raise ViewerError("contour rgba must be 3 or 4 numbers in [0, 1]")
        if int(index_every) < 0:
            raise ViewerError(f"index_every must be >= 0, got {index_every}")
        self._contours = {"interval": interval, "base": base, "width": width, "rgba": tuple(float(c) for c in colour),
                          "index_every": int(index_every), "index_width": index_width}
        self._revision += 1

    def disable_contours(self) -> None:
        self._contours = None
        self._revision += 1

    def enable_streams(self, threshold: int, *, width: float = 1.5, rgba=(0.1, 0.3, 0.8, 1.0), trunk_threshold: int = 0,
                       trunk_width: float = 3.0, fill: bool = False) -> None:
        """The stream network of the terrain as it is rendered -- every sample whose D8 flow accumulation reaches ``threshold``
        samples, joined to its receiver --, painted on the GPU from the session's own tables (TerrainSession.paint_streams)
        after the contour lines and before the vector layers.  ``width`` and ``trunk_width`` are stroke widths in canvas
        texels; ``trunk_threshold`` > 0 paints the network of that higher accumulation a second time ``trunk_width`` wide (the
        index contours' idiom).  ``rgba``: linear colour and alpha.  ``fill=True`` routes over the filled surface
        (TerrainSession.fill): the rivers cross every lake and flat and reach the border."""
        width, trunk_width = float(width), float(trunk_width)
        if int(threshold) != threshold or int(threshold) < 1 or int(trunk_threshold) != trunk_threshold or int(trunk_threshold) < 0:
            raise ViewerError(f"stream thresholds are accumulations: threshold >= 1 and trunk_threshold >= 0, got {threshold} and {trunk_threshold}")
        if not (np.isfinite(width) and width >= 0.0 and np.isfinite(trunk_width) and trunk_width >= 0.0):
            raise ViewerError(f"stream widths must be finite and >= 0 texels, got {width} and {trunk_width}")
        colour = np.asarray(rgba, np.float32).reshape(-1)
        if colour.shape[0] not in (3, 4) or not np.all((colour >= 0.0) & (colour <= 1.0)):
            raise ViewerError("stream rgba must be 3 or 4 numbers in [0, 1]")
        self._streams = {"threshold": int(threshold), "width": width, "rgba": tuple(float(c) for c in colour),
                         "trunk_threshold": int(trunk_threshold), "trunk_width": trunk_width, "fill": bool(fill)}
        self._revision += 1

    def disable_streams(self) -> None:
        self._streams = None
        self._revision += 1

    def _painted(self) -> bool:
        """Does the scene need a painted canvas: contour lines, streams or vector layers?"""
        return self._contours is not None or self._streams is not None or bool(self.vector_layers())

    def _paint_layers(self, s, keywords) -> None:
        """Drape ``s`` with the constant canvas unless an overlay image is there already, then paint the contour lines, over
        them the streams and, over those, the layers."""
        layers = self.vector_layers()
        if not self._painted():
            return
        if not s.draped:
            rows, cols = self.vector_canvas_shape(s.dem_shape)
            albedo = np.asarray(keywords.get("albedo", (0.6, 0.6, 0.6)), np.float32)
            s.drape(np.broadcast_to(albedo, (rows, cols, 3)), filter="bilinear", registration="area")
        info = s.drape_info()
        sx, _, sz, _ = (self.overlay_registration(s.dem_shape, self._overlay["image"].shape, self._overlay["extent"])
                        if self._overlay is not None else s.drape_registration(info["rows"], info["cols"], "area"))
        spacing = keywords.get("spacing", (1.0, 1.0))
        texel = max(abs(float(spacing[0]) / float(sx)), abs(float(spacing[1]) / float(sz)))  # one canvas texel in metres
        c = self._contours
        if c is not None:
            levels = s.contour_levels(c["interval"], c["base"])
            s.paint_contours(levels, rgba=c["rgba"], width=c["width"] * texel)
            if c["index_every"] > 0:
                k = np.rint((levels.astype(np.float64) - c["base"]) / c["interval"]).astype(np.int64)
                index = levels[k % c["index_every"] == 0]
                if index.size:
                    s.paint_contours(index, rgba=c["rgba"], width=c["index_width"] * texel)
        w = self._streams
        if w is not None:
            s.paint_streams(w["threshold"], rgba=w["rgba"], width=w["width"] * texel, fill=w["fill"])
            if w["trunk_threshold"] > 0:
                s.paint_streams(w["trunk_threshold"], rgba=w["rgba"], width=w["trunk_width"] * texel, fill=w["fill"])
        for layer in layers:
            s.paint(layer["xz"], layer["rgba"], layer["indices"], primitive=layer["primitive"], width=layer["texels"] * texel,
                    opacity=layer["opacity"], features=layer["features"])

    def render(self, width: Optional[int] = None, height: Optional[int] = None) -> dict:
        """OfflineTerrainViewer.render; with an overlay or vector layers loaded, the same loop on a session draped with them."""
        overlay = getattr(self, "_overlay", None)
        if overlay is None and not self._painted():
            return super().render(width, height)
        dem, w, h, camera, keywords = self._call(width, height)
        with self._draped_session(dem, w, h, camera, keywords) as s:
            self.last_result = s.render()
        return self.last_result

    def _draped_session(self, dem, w, h, camera, keywords):
        """A session of the viewer's scene, draped with the loaded overlay, the vector layers painted over it."""
        from .session import TerrainSession

        overlay = self._overlay
        s = TerrainSession(dem, w, h, camera, **keywords)
        try:
            if overlay is not None:
                reg = self.overlay_registration(s.dem_shape, overlay["image"].shape, overlay["extent"])
                s.drape(overlay["image"], filter=overlay["filter"], registration=reg, srgb=overlay["srgb"])
            self._paint_layers(s, keywords)
        except Exception:
            s.close()
            raise
        return s

    # -- output -------------------------------------------------------------------------------------------
    def _call(self, width: Optional[int] = None, height: Optional[int] = None):
        if not self._open:
            raise ViewerError("viewer is closed")
        self._render.update(env_map=self._env, env_intensity=self._env_intensity, sun_intensity=self._sun_intensity)
        return super()._call(width, height)

    def render_animation(self, animation: Sequence[Mapping[str, Any]], output_dir: Union[str, Path], fps: int = 30,
                         width: Optional[int] = None, height: Optional[int] = None, progress_callback=None) -> None:
        """A sequence of camera keyframes ({"phi_deg", "theta_deg", "radius"[, "fov_deg", "target"]} per frame),
        one PNG per frame named frame_0000.png ... like the reference's exporter (viewer.py:1270-1334); the DEM's
        acceleration tables are built once (the library's scene cache) and ONE session renders every frame, re-aimed per
        key (path_tracing.render_terrain_camera_sequence): each PNG is what ``snapshot()`` under that key writes."""
        from .path_tracing import render_terrain_camera_sequence

        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        if self._overlay is not None or self._painted():  # (a draped scene: ONE session draped and painted, re-aimed per key)
            session = None
            try:
                for i, key in enumerate(animation):
                    self.set_orbit_camera(key["phi_deg"], key["theta_deg"], key["radius"], key.get("fov_deg"), key.get("target"))
                    dem, w, h, camera, keywords = self._call(width, height)
                    if session is None:
                        session = self._draped_session(dem, w, h, camera, keywords)
                    else:
                        session.reaim(camera)
                    self.last_result = session.render()
                    _io.numpy_to_png(out / f"frame_{i:04d}.png", self.last_result["rgba"])
                    if progress_callback:
                        progress_callback(i, len(animation))
            finally:
                if session is not None:
                    session.close()
            return
        frames, call = [], None
        for key in animation:
            self.set_orbit_camera(key["phi_deg"], key["theta_deg"], key["radius"], key.get("fov_deg"), key.get("target"))
            call = self._call(width, height)
            frames.append({"camera": call[3]})
        if call is None:
            return
        dem, w, h, _, keywords = call
        for i, result in enumerate(render_terrain_camera_sequence(dem, w, h, frames=frames, **keywords)):
            self.last_result = result
            _io.numpy_to_png(out / f"frame_{i:04d}.png", result["rgba"])
            if progress_callback:
                progress_callback(i, len(animation))

    def pick_at(self, x: int, y: int, *, shift: bool = False, ctrl: bool = False) -> list:
        """What lies under pixel (x, y) of the viewer's current scene and camera (reference viewer.py:910): one closest-hit
        ray through the pixel's centre on a session of that scene (TerrainSession.pick) -- ``[{"kind": "terrain" | "mesh",
        "world_pos": [x, y, z], "distance": t, "normal": [...], "primitive": int}]``, or ``[]`` for sky.  ``shift`` / ``ctrl``
        (the raster viewer's selection modifiers) are accepted and ignored.  Parity with the reference is NOT pinned: its
        pick reads the frozen frame of its raster viewer (feature ids, f64 viewer-world positions); this one is the path
        tracer's own centre ray, exact for what the path tracer renders."""
        from .session import TerrainSession

        _ = shift, ctrl
        dem, w, h, camera, keywords = self._call()
        if not (0 <= int(x) < w and 0 <= int(y) < h):
            raise ViewerError(f"pick_at({x}, {y}) is outside the {w}x{h} viewport")
        with TerrainSession(dem, w, h, camera, **keywords) as s:
            hit = s.pick(np.array([[int(x), int(y)]], np.uint32))
        kind = int(hit["kind"][0])
        if kind == 0:
            return []
        return [{"kind": "terrain" if kind == 1 else "mesh", "world_pos": [float(v) for v in hit["position"][0]],
                 "distance": float(hit["t"][0]), "normal": [float(v) for v in hit["normal"][0]], "primitive": int(hit["primitive"][0])}]

    def get_stats(self) -> Dict[str, Any]:
        last = self.last_result or {}
        return {"applied_command_revision": self._revision, "rendered_revision": self._revision, "frames": last.get("frames"),
                "variance": last.get("variance"), "gpu_resource_bytes": last.get("gpu_resource_bytes"), "backend": "hip-gfx950"}

    def send_ipc(self, cmd: Dict[str, Any]) -> Dict[str, Any]:
        raise ViewerError("the offline path tracer has no IPC channel; call the methods directly")

    def close(self) -> None:
        self._open = False

    def __enter__(self) -> "ViewerHandle":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    @property
    def is_running(self) -> bool:
        return self._open

    def __getattr__(self, name):
        if name in _RASTER_ONLY:
            def refuse(*_a, **_k):
                raise ViewerError(f"ViewerHandle.{name} belongs to the interactive raster viewer; the offline path "
                                  "tracer has no counterpart")
            return refuse
        raise AttributeError(name)


def open_viewer_async(width: int = 1280, height: int = 720, title: str = "forge3d Interactive Viewer", obj_path=None,
                      gltf_path=None, terrain_path=None, fov_deg: float = 60.0, timeout: float = 30.0,
                      ipc_host: str = "127.0.0.1", ipc_port: int = 0) -> ViewerHandle:
    """reference viewer.py:1390-1517 -- returns at once with a handle; here there is nothing to launch."""
    _ = title, timeout, ipc_host, ipc_port
    if obj_path is not None or gltf_path is not None:
        raise ViewerError("the offline path tracer renders terrain (and meshes passed to hybrid_render_terrain_reference); "
                          "OBJ / glTF scenes belong to the raster viewer")
    handle = ViewerHandle(width, height, fov_deg=fov_deg)
    if terrain_path is not None:
        handle.load_terrain(terrain_path)
    return handle


def open_viewer(*args, **kwargs) -> ViewerHandle:
    """reference viewer.py:1519-: the blocking variant; offline there is nothing to block on."""
    return open_viewer_async(*args, **kwargs)


class Renderer:
    """``forge3d.Renderer(width, height)`` (reference python/forge3d/__init__.py:347-421): the reference's class is a
    deterministic CPU stub (`render_triangle_rgba`); its constructor / ``get_config`` shape is kept and
    ``render_terrain`` routes a DEM to the path tracer."""

    def __init__(self, width: int, height: int, *, config: "Mapping[str, Any] | None" = None, **kwargs: Any) -> None:
        self.width, self.height = int(width), int(height)
        allowed = {"exposure", "spp", "max_frames", "min_frames", "variance_threshold", "seed"}
        unexpected = sorted(k for k in kwargs if k not in allowed)
        if unexpected:
            raise TypeError(f"Unexpected arguments: {', '.join(unexpected)}")
        self._config = {"backend": "hip-gfx950", "lighting": {"exposure": float(kwargs.pop("exposure", 1.0))},
                        "path_tracing": {"spp": 8, "max_frames": 512, "min_frames": 32, "variance_threshold": 1e-3, "seed": 7}}
        if config:
            self._config.update({k: v for k, v in dict(config).items()})
        self._config["path_tracing"].update(kwargs)

    def get_config(self) -> dict:
        return {k: (dict(v) if isinstance(v, dict) else v) for k, v in self._config.items()}

    def render_triangle_rgba(self, *, certificate=False, cache=None) -> np.ndarray:
        """The reference's deterministic test pattern (__init__.py:382-407), vectorised."""
        y, x = np.mgrid[0:self.height, 0:self.width]
        cx, cy, size = self.width // 2, self.height // 2, min(self.width, self.height) // 4
        inside = (np.abs(x - cx) + np.abs(y - cy) < size) & (y > cy - size // 2)
        img = np.empty((self.height, self.width, 4), np.uint8)
        img[...] = (16, 16, 24, 255)
        img[inside] = (128, 64, 32, 255)
        return img

    def render_triangle_png(self, path, *, certificate=False, cache=None) -> None:
        _io.numpy_to_png(path, self.render_triangle_rgba())

    def render_terrain(self, heightmap, camera=None, **kwargs) -> dict:
        from .path_tracing import hybrid_render_terrain_reference

        cam = dict(camera or {})
        cam.setdefault("exposure", self._config["lighting"]["exposure"])
        return hybrid_render_terrain_reference(heightmap, self.width, self.height, cam,
                                               **{**self._config["path_tracing"], **kwargs})
