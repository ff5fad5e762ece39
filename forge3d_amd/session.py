"""Steppable, device-resident form of the terrain render (C ABI ``f3d_session_*``).

Used by bench.py (inputs resident in HBM before the timed region) and by the row-strip
multi-GPU driver (forge3d_amd/distributed.py).  One TerrainSession owns the image rows
[row_begin, row_end); RNG and all state are keyed by full-image coordinates.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

HALO_ROWS = 4  # f3d_scene.h kHaloRows: the spatial pass reaches [-3, +4] rows
RESERVOIR_BYTES = 16
WELFORD_WINDOW = 32


# What the raster and query methods share in front of the library.  An input is a NumPy array (the host form) or a torch
# tensor (the device form); a method decides the form ONCE (_form) and hands the device down -- None is the host form -- and
# every output comes back in the input's form.
def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


_torch = None  # the torch module and, per NumPy dtype of an output, the tensor dtype with its bits: set when the first tensor comes in
_TENSOR_BITS = {}


def _form(x, wait, noun, plural, device=None):
    """The form of a call whose input is ``x``: the device the outputs go to for a tensor (or ``device``, for a call without
    an input), None for the host form -- with the two refusals of a form, raised before anything is converted or allocated."""
    global _torch
    if device is None and (x is None or isinstance(x, np.ndarray) or type(x).__module__.split(".")[0] != "torch"):
        if not wait:
            raise ValueError(f"wait=False is for tensor {plural}: results in host memory are there when the call returns")
        return None
    if x is not None and not x.is_cuda:
        raise ValueError(f"a tensor {noun} needs a tensor on the session's device (NumPy arrays take the host form)")
    if _torch is None:
        import torch  # (only for callers who hand tensors in)

        _TENSOR_BITS.update({np.float32: torch.float32, np.uint32: torch.int32, np.uint64: torch.int64, np.uint8: torch.uint8})
        _torch = torch
    return x.device if device is None else device


def _rows4(rows, device):
    """(K, 3) or (K, 4) rows as contiguous float32 (K, 4), the missing column 0; a tensor (``device`` not None) stays one."""
    if device is not None:
        t = rows.to(_torch.float32)
    else:
        t = np.asarray(rows, dtype=np.float32)
    if t.ndim != 2 or t.shape[1] not in (3, 4):
        raise ValueError(f"expected shape (K, 4) or (K, 3), got {tuple(t.shape)}")
    if device is not None:
        return (_torch.cat([t, _torch.zeros_like(t[:, :1])], 1) if t.shape[1] == 3 else t).contiguous()
    return np.ascontiguousarray(np.concatenate([t, np.zeros((t.shape[0], 1), np.float32)], 1) if t.shape[1] == 3 else t)


def _output(device, want, shape, dtype):
    """An output of ``shape`` and NumPy ``dtype``, None unless ``want``: NumPy zeros for the host form, an uninitialised tensor
    on ``device`` for the device form (the kernel writes every element; uint32 is int32 bits, uint64 int64 bits)."""
    if not want:
        return None
    return np.zeros(shape, dtype) if device is None else _torch.empty(shape, dtype=_TENSOR_BITS[dtype], device=device)


def _stroke(rgba, width, opacity):
    """The stroke of a paint call, checked: ``(one RGBA colour as float32 -- three numbers: alpha 1; None for ``rgba=None``, the
    caller's own colours --, the float32 half-width, the opacity)``."""
    col = None
    if rgba is not None:
        col = np.asarray(rgba, dtype=np.float32).reshape(-1)
        if col.shape[0] not in (3, 4):
            raise ValueError(f"rgba must be one colour of 3 or 4 numbers, got {np.shape(rgba)}")
        if col.shape[0] == 3:
            col = np.concatenate([col, np.ones(1, np.float32)])
    width, opacity = float(width), float(opacity)
    if not np.isfinite(width) or width < 0.0:
        raise ValueError(f"width must be finite and >= 0 metres, got {width}")
    if not 0.0 <= opacity <= 1.0:
        raise ValueError(f"opacity must lie in [0, 1], got {opacity}")
    return col, np.float32(width) * np.float32(0.5), opacity


class FilledRouting:
    """``TerrainSession.filled``: the session's drainage calls with F3D_DRAINAGE_FILL set."""

    def __init__(self, session):
        self._session = session

    def drainage(self, region=None, *, direction=True, accumulation=True, basin=False, out=None):
        return self._session._drainage(region, direction, accumulation, basin, out, True)

    def flow_directions(self, region=None):
        return self.drainage(region, direction=True, accumulation=False)["direction"]

    def flow_accumulation(self, region=None):
        return self.drainage(region, direction=False, accumulation=True)["accumulation"]

    def basins(self, region=None):
        return self.drainage(region, direction=False, accumulation=False, basin=True)["basin"]

    def streams(self, threshold, *, region=None, out=None):
        return self._session._streams(threshold, region, out, True)

    def paint_streams(self, threshold, **style):
        return self._session.paint_streams(threshold, fill=True, **style)


class TerrainSession:
    def __init__(self, heightmap, width, height, camera=None, *, row_begin=0, row_end=0, device=-1, stream=0,
                 memory_budget_bytes=0, kernel_variant=0, ext_reservoirs=(None, None), ext_stats=None, bands=0,
                 band_streams=0, mesh_builder=0, frames_in_flight=0,
                 spacing=(1.0, 1.0), exaggeration=1.0, albedo=(0.6, 0.6, 0.6), sun_azimuth_deg=315.0,
                 sun_elevation_deg=45.0, sun_intensity=2.5, sun_color=(1.0, 0.97, 0.92), env_map=None,
                 env_intensity=0.35, mesh_vertices=None, mesh_indices=None, spp=1, max_frames=512, min_frames=32,
                 variance_threshold=1e-3, seed=7, observer_latitude_deg=0.0, observer_longitude_deg=0.0,
                 earth_model="ellipsoid", sphere_radius_m=6_371_008.8, refraction_model="bennett",
                 refraction_k=0.13, pressure_mbar=1013.25, temperature_c=15.0, atmosphere=None):
        self._lib = _native.lib()
        self._handle = C.c_void_p(None)
        desc, keep = _native.make_desc(heightmap, width, height, dict(camera or {}), spacing, exaggeration, albedo,
                                       sun_azimuth_deg, sun_elevation_deg, sun_intensity, env_map, env_intensity,
                                       mesh_vertices, mesh_indices, spp, max_frames, min_frames,
                                       variance_threshold, seed, sun_color, observer_latitude_deg,
                                       observer_longitude_deg, earth_model, sphere_radius_m, refraction_model,
                                       refraction_k, pressure_mbar, temperature_c, atmosphere)
        opts = _native.SessionOpts()
        opts.struct_size = C.sizeof(_native.SessionOpts)
        opts.device = int(device)
        opts.stream = C.c_void_p(int(stream) or None)
        opts.row_begin, opts.row_end = int(row_begin), int(row_end)
        opts.memory_budget_bytes = int(memory_budget_bytes)
        opts.kernel_variant = int(kernel_variant)
        opts.ext_reservoirs[0] = C.c_void_p(ext_reservoirs[0] or None)
        opts.ext_reservoirs[1] = C.c_void_p(ext_reservoirs[1] or None)
        opts.ext_stats = C.c_void_p(ext_stats or None)
        opts.bands, opts.band_streams = int(bands), int(band_streams)
        opts.mesh_builder = int(mesh_builder)
        opts.frames_in_flight = int(frames_in_flight)
        err = C.create_string_buffer(1024)
        rc = self._lib.f3d_session_create(C.byref(desc), C.byref(opts), C.byref(self._handle), err, len(err))
        del keep
        if rc != 0:
            self._handle = C.c_void_p(None)
            _native.raise_status(rc, err.value.decode("utf-8", "replace"))
        self.width, self.height = int(width), int(height)
        self._device = int(device)
        # what rearm() keeps when a value is not given: the descriptor's re-armable members as the library holds them
        self._armed = {"sun_azimuth_deg": float(desc.sun_azimuth_deg), "sun_elevation_deg": float(desc.sun_elevation_deg),
                       "sun_intensity": float(desc.sun_intensity), "sun_color": tuple(float(c) for c in desc.sun_color),
                       "exposure": float(desc.exposure), "env_intensity": float(desc.env_intensity), "seed": int(desc.seed),
                       "max_frames": int(desc.max_frames), "min_frames": int(desc.min_frames),
                       "variance_threshold": float(desc.variance_threshold),
                       "observer_latitude_deg": float(desc.observer_latitude_deg),
                       "observer_longitude_deg": float(desc.observer_longitude_deg),
                       "pressure_mbar": float(desc.pressure_mbar), "temperature_c": float(desc.temperature_c)}
        self._camera = dict(camera or {})  # what remesh() and reterrain() keep when no camera is given
        # what ground() starts its vertical rays above: upper bounds of the terrain's and the mesh's highest point, kept up
        # by reterrain() / remesh() (a bound only has to be above the scene: a lowered summit leaves it where it was)
        dem = np.asarray(heightmap, dtype=np.float32)
        self._exaggeration = float(desc.exaggeration)
        self._terrain_top = float(dem.max()) * self._exaggeration
        self._terrain_bottom = float(dem.min()) * self._exaggeration  # (a lower bound, kept like the upper one: contour_levels())
        self._mesh_top = float(np.asarray(mesh_vertices, dtype=np.float32)[:, 1].max()) if mesh_vertices is not None else None
        self.dem_shape = (int(desc.dem_height), int(desc.dem_width))
        self.row_begin = int(row_begin)
        self.row_end = int(row_end) or int(height)
        self.rows = self.row_end - self.row_begin
        self.spp = int(spp)
        self._err = err

    # -- lifecycle --------------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.f3d_session_destroy(self._handle)
            self._handle = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            _native.raise_status(rc, self._err.value.decode("utf-8", "replace"))

    # -- re-arm: another render on this session ---------------------------------------
    REARMABLE = ("sun_azimuth_deg", "sun_elevation_deg", "sun_intensity", "sun_color", "exposure", "env_intensity", "seed",
                 "max_frames", "min_frames", "variance_threshold", "observer_latitude_deg", "observer_longitude_deg",
                 "pressure_mbar", "temperature_c")

    def rearm(self, *, sun_azimuth_deg=None, sun_elevation_deg=None, sun_intensity=None, sun_color=None, exposure=None,
              env_intensity=None, seed=None, max_frames=None, min_frames=None, variance_threshold=None,
              observer_latitude_deg=None, observer_longitude_deg=None, pressure_mbar=None, temperature_c=None):
        """Make the next frames a new render under another sun / seed / exposure / IBL intensity / frame budget (None keeps
        the current value): what a new session with these values renders, without its set-up.  Asynchronous on the
        session stream, behind everything enqueued so far; a refused value leaves the session as it was."""
        given = dict(locals())
        given.pop("self")
        r = self._rearm_desc(given)
        self._update(self._lib.f3d_session_rearm, r, r)

    def reaim(self, camera=None, **rearmable):
        """rearm() under a new camera: what ``TerrainSession(..., camera=camera, **values)`` renders, on this session.
        ``camera`` is read exactly as the constructor reads it (a missing ``origin`` / ``look_at`` / ``up`` / ``fov_y`` /
        ``exposure`` takes the wrapper's default, not the session's current value; an ``exposure=`` keyword wins over the
        dict's); the other values as rearm() takes them (not given: kept).  One pass traces the centre rays again and
        clears the per-render state; same contract as rearm().  Without a camera this is rearm()."""
        if camera is None:
            return self.rearm(**rearmable)
        self._known("reaim", rearmable)
        a = self._aim(camera, rearmable)
        self._update(self._lib.f3d_session_reaim, a, a.arm, camera)

    def remesh(self, mesh_vertices, mesh_indices=None, camera=None, **rearmable):
        """reaim() under a moved or another mesh: what ``TerrainSession(..., mesh_vertices=..., mesh_indices=..., camera=camera,
        **values)`` renders, on this session.  Without ``mesh_indices`` the vertices (the session's count) move the
        session's mesh: uploaded in stream order, the BVH refitted on the GPU -- no host build, no wait, nothing allocated
        after the first call; the tree keeps its topology, so large motion costs walk time, never the image.  With
        ``mesh_indices`` (the same ones for a fresh tree, or another mesh) the create's path runs.  ``camera`` None keeps the
        current one (and the current exposure); otherwise it is read as reaim() reads it.  Same contract as reaim(): a
        refused value leaves the session as it was, rendering the old mesh."""
        self._known("remesh", rearmable)
        mv = np.ascontiguousarray(mesh_vertices, dtype=np.float32)
        if mv.ndim != 2 or mv.shape[1] != 3:
            raise ValueError("mesh_vertices must have shape (N, 3)")
        m = _native.RemeshDesc()
        m.struct_size = C.sizeof(_native.RemeshDesc)
        m.mesh_vertices, m.mesh_vertex_count = mv.ctypes.data, mv.shape[0]
        if mesh_indices is not None:
            mi = np.ascontiguousarray(mesh_indices, dtype=np.uint32)
            if mi.ndim != 2 or mi.shape[1] != 3:
                raise ValueError("mesh_indices must have shape (M, 3)")
            m.mesh_indices, m.mesh_index_count = mi.ctypes.data, mi.size
        m.aim = self._aim(camera, rearmable)
        self._update(self._lib.f3d_session_remesh, m, m.aim.arm, camera)  # (mv and mi live until here)
        self._mesh_top = float(mv[:, 1].max())

    def reterrain(self, heightmap, camera=None, *, at=None, exaggeration=None, **rearmable):
        """reaim() under new DEM samples: what ``TerrainSession(resulting_dem, ..., camera=camera, exaggeration=..., **values)``
        renders, on this session.  ``heightmap`` is the whole DEM (``at`` None: it must have the session's DEM shape) or a 2-D
        patch whose first sample lies at DEM sample ``at=(row, col)``.  The samples are uploaded in stream order and the
        session's own acceleration tables are patched on the GPU over the patch's footprint -- no host hash, no table build,
        no wait, nothing allocated after the first call of a patch size.  ``exaggeration`` None keeps the session's; another
        value rescales every sample and needs the whole DEM.  ``camera`` None keeps the current one (and the current
        exposure); otherwise it is read as reaim() reads it.  DEM size and spacing stay the session's.  Same contract as
        reaim(): a refused value leaves the session as it was, rendering the old terrain."""
        self._known("reterrain", rearmable)
        block = np.ascontiguousarray(heightmap, dtype=np.float32)
        if block.ndim != 2:
            raise ValueError(f"heightmap must be 2D (H, W), got shape {block.shape}")
        if at is None:
            if block.shape != self.dem_shape:
                raise ValueError(f"heightmap has shape {block.shape}, the session's DEM has {self.dem_shape}: a patch needs at=(row, col), "
                                 "another DEM size needs a new session")
            row, col = 0, 0
        else:
            row, col = (int(v) for v in at)
            if row < 0 or col < 0:
                raise ValueError(f"at=(row, col) must not be negative, got {tuple(at)}")
        t = _native.ReterrainDesc()
        t.struct_size = C.sizeof(_native.ReterrainDesc)
        t.heights = block.ctypes.data
        t.height, t.width = block.shape
        t.y0, t.x0 = row, col
        t.exaggeration = 0.0 if exaggeration is None else float(exaggeration)
        if exaggeration is not None and float(exaggeration) == 0.0:
            t.exaggeration = float("nan")  # (0 means "keep" in the C ABI; a zero exaggeration is the create's refusal)
        t.aim = self._aim(camera, rearmable)
        self._update(self._lib.f3d_session_reterrain, t, t.aim.arm, camera)  # (block lives until here)
        if exaggeration is not None:  # (accepted only with the whole DEM: the bound is exact again)
            self._exaggeration = float(np.float32(exaggeration))
            self._terrain_top = float(block.max()) * self._exaggeration
            self._terrain_bottom = float(block.min()) * self._exaggeration
        else:
            self._terrain_top = max(self._terrain_top, float(block.max()) * self._exaggeration)
            self._terrain_bottom = min(self._terrain_bottom, float(block.min()) * self._exaggeration)

    # -- drape: an image laid over the terrain, per-texel albedo -----------------------------------
    DRAPE_FILTERS = {"nearest": _native.DRAPE_NEAREST, "bilinear": _native.DRAPE_BILINEAR}

    def drape_registration(self, rows: int, cols: int, registration="area"):
        """The four f32 numbers ``(scale_x, offset_x, scale_z, offset_z)`` that take DEM-sample coordinates to texel coordinates
        (``t = f * scale + offset``) for an image of ``rows x cols`` texels: ``"area"`` -- the image covers the DEM's extent edge
        to edge, ``scale = cols / (w - 1)``, ``offset = -0.5``; ``"point"`` -- texel centres sit on the corresponding fraction of
        samples, ``scale = (cols - 1) / (w - 1)``, ``offset = 0``; or four numbers of the caller's, taken as given."""
        dem_h, dem_w = self.dem_shape
        if isinstance(registration, str):
            if registration == "area":
                reg = (cols / (dem_w - 1), -0.5, rows / (dem_h - 1), -0.5)
            elif registration == "point":
                reg = ((cols - 1) / (dem_w - 1), 0.0, (rows - 1) / (dem_h - 1), 0.0)
            else:
                raise ValueError(f"registration must be 'area', 'point' or (scale_x, offset_x, scale_z, offset_z), got {registration!r}")
        else:
            reg = tuple(float(v) for v in registration)
            if len(reg) != 4:
                raise ValueError(f"registration must be 'area', 'point' or (scale_x, offset_x, scale_z, offset_z), got {registration!r}")
        reg = tuple(np.float32(v) for v in reg)
        if not all(np.isfinite(v) for v in reg) or reg[0] == 0 or reg[2] == 0:
            raise ValueError(f"registration numbers must be finite and the scales non-zero, got {tuple(float(v) for v in reg)} "
                             "(a one-texel image under 'point' has no extent: use 'area')")
        return reg

    def drape(self, image, camera=None, *, filter="bilinear", registration="area", at=None, srgb=False, wait=True, **rearmable):
        """reaim() under an image laid over the terrain: the albedo of terrain hits becomes the image's texel under the hit point
        (mesh hits keep theirs, the sky is untouched), per sample, and the albedo AOV the image at the centre ray's hit.
        ``image`` is ``(H, W, 3|4)`` linear RGB reflectances (a fourth channel is ignored), row 0 on DEM row 0 and column 0 on
        DEM column 0 -- the heightmap's orientation: a NumPy float32 array, a uint8 array (divided by 255), a float32 tensor
        on the session's device (nothing copied; ``wait=False`` returns with the packing kernel in flight on the session's
        stream), or ``None``, which removes the drape -- every later output is then bit-identical to a session that never had
        one.  ``srgb=True`` decodes a NumPy image to linear first.  ``filter``: ``"bilinear"`` (clamp to edge) or ``"nearest"``.
        ``registration``: see drape_registration().  ``at=(row, col)`` overwrites that window of the session's drape with
        ``image`` (a time-lapse of imagery without uploading all of it again): size, filter and registration stay.
        Texels are stored as binary16; a host image with a non-finite, negative or > 65504 value is refused, a tensor's such
        values are stored as 0.  ``camera`` None keeps the current one (and the current exposure); otherwise it is read as
        reaim() reads it.  Same contract as reaim(): the render restarts at frame 0 and a refused value leaves the session as
        it was, rendering the old drape.  Frames in flight, the register-budget A/B kernel variants and connected peer halos
        have no draped form: such a session refuses a drape."""
        self._known("drape", rearmable)
        q = _native.DrapeDesc()
        q.struct_size = C.sizeof(_native.DrapeDesc)
        keep = None
        if image is None:
            if at is not None:
                raise ValueError("image=None removes the drape: it takes no at=(row, col)")
        else:
            if filter not in self.DRAPE_FILTERS:
                raise ValueError(f"filter must be 'nearest' or 'bilinear', got {filter!r}")
            if type(image).__module__.split(".")[0] == "torch":
                import torch  # (only for callers who hand tensors in)

                if not image.is_cuda:
                    raise ValueError("a tensor drape needs a tensor on the session's device (NumPy arrays take the host form)")
                if image.dtype != torch.float32:
                    raise ValueError(f"a tensor drape must be float32, got {image.dtype}")
                if srgb:
                    raise ValueError("srgb=True decodes a NumPy image: decode a tensor before handing it in")
                if image.ndim != 3 or image.shape[2] not in (3, 4):
                    raise ValueError(f"image must have shape (H, W, 3) or (H, W, 4), got {tuple(image.shape)}")
                if not wait and not image.is_contiguous():
                    raise ValueError("wait=False needs a contiguous tensor: the packing kernel reads the caller's memory after the call "
                                     "returns, and a copy made here would be gone by then")
                keep = image.contiguous()
                shape = tuple(int(v) for v in keep.shape)
                q.image = keep.data_ptr() if keep.numel() else None
                q.flags = _native.DRAPE_DEVICE_POINTERS | (0 if wait else _native.DRAPE_NO_WAIT)
            else:
                arr = np.asarray(image)
                if arr.ndim != 3 or arr.shape[2] not in (3, 4):
                    raise ValueError(f"image must have shape (H, W, 3) or (H, W, 4), got {arr.shape}")
                if arr.dtype == np.uint8:
                    arr = arr.astype(np.float32) / np.float32(255.0)
                elif arr.dtype != np.float32:
                    raise ValueError(f"image must be float32 or uint8, got {arr.dtype}")
                if srgb:
                    arr = srgb_to_linear(arr)
                if not wait:
                    raise ValueError("wait=False is for tensor images: an image in host memory has been read when the call returns")
                keep = np.ascontiguousarray(arr, dtype=np.float32)
                shape = keep.shape
                q.image = keep.ctypes.data if keep.size else None
            if shape[0] == 0 or shape[1] == 0:
                raise ValueError(f"image is empty: shape {shape}")
            q.rows, q.cols, q.channels = shape
            if at is None:
                q.filter = self.DRAPE_FILTERS[filter]
                q.scale_x, q.offset_x, q.scale_z, q.offset_z = self.drape_registration(shape[0], shape[1], registration)
            else:
                row, col = (int(v) for v in at)
                if row < 0 or col < 0:
                    raise ValueError(f"at=(row, col) must not be negative, got {tuple(at)}")
                q.at_row, q.at_col = row, col
                q.flags |= _native.DRAPE_PATCH
        q.aim = self._aim(camera, rearmable)
        self._update(self._lib.f3d_session_drape, q, q.aim.arm, camera)  # (keep lives until here)
        del keep

    @property
    def draped(self) -> bool:
        """Does the session hold a drape?"""
        return bool(self._lib.f3d_session_draped(self._handle, None))

    def drape_info(self):
        """``None`` without a drape, else ``{"rows", "cols", "filter", "bytes"}`` of the one the session holds."""
        info = (C.c_uint32 * 4)()
        if not self._lib.f3d_session_draped(self._handle, info):
            return None
        names = {v: k for k, v in self.DRAPE_FILTERS.items()}
        return {"rows": int(info[0]), "cols": int(info[1]), "filter": names[int(info[2])], "bytes": int(info[3])}

    # -- paint: vector features composited into the drape, on the GPU ---------------------------------
    PAINT_PRIMITIVES = {"points": _native.PAINT_POINTS, "lines": _native.PAINT_LINES, "triangles": _native.PAINT_TRIANGLES}

    @staticmethod
    def paint_indices(count: int, primitive: str):
        """The index list ``indices=None`` stands for over ``count`` vertices: every vertex for points, one strip for lines,
        consecutive triples for triangles."""
        if primitive == "lines":
            i = np.arange(max(count - 1, 0), dtype=np.uint32)
            return np.stack([i, i + np.uint32(1)], 1).ravel()
        return np.arange(count - (count % 3 if primitive == "triangles" else 0), dtype=np.uint32)

    def paint(self, xz, rgba, indices=None, *, primitive="lines", width=1.0, opacity=1.0, features=None, camera=None, **rearmable):
        """reaim() over a drape with vector features painted into it: roads, rivers, parcels, tracks, markers, rasterised on the
        GPU into the session's drape (drape() gives the canvas first), which the frames then sample as before.  ``xz`` is
        ``(N, 2)`` world x, z; ``rgba`` one colour or ``(N, 4)`` colours, linear RGB reflectance and alpha in [0, 1] (three numbers:
        alpha 1); ``indices`` index the vertices, 1 / 2 / 3 a primitive (``None``: see paint_indices()).  ``primitive``:
        ``"lines"`` -- strokes ``width`` metres wide with round caps and joins and a one-texel edge ramp, ``"points"`` -- discs of
        diameter ``width``, ``"triangles"`` -- filled, watertight across shared edges.  ``features`` is ``(N,)`` feature ids: a run
        of consecutive primitives whose first vertices carry one id is one feature and blends once (no darker joints under
        ``opacity`` < 1); without ids the whole call is one feature.  Features blend in list order, the later over the earlier.
        Coordinates lie within 65536 canvas texels of the terrain's centre (the world's origin): the reach the rasteriser's f32
        distances are sized for; clip far geometry to the terrain's neighbourhood.
        ``camera`` and the other values as reaim() takes them.  Same contract as drape(): the render restarts at frame 0 and a
        refused value leaves the session, and the canvas, as they were."""
        self._known("paint", rearmable)
        if primitive not in self.PAINT_PRIMITIVES:
            raise ValueError(f"primitive must be 'points', 'lines' or 'triangles', got {primitive!r}")
        pts = np.ascontiguousarray(xz, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] == 0:
            raise ValueError(f"xz must have shape (N, 2) with N >= 1, got {pts.shape}")
        n = pts.shape[0]
        col = np.asarray(rgba, dtype=np.float32)
        if col.ndim == 1 and col.shape[0] in (3, 4):
            col = np.broadcast_to(col, (n, col.shape[0]))
        if col.ndim != 2 or col.shape[0] != n or col.shape[1] not in (3, 4):
            raise ValueError(f"rgba must be one colour of 3 or 4 numbers or have shape ({n}, 3|4), got {np.shape(rgba)}")
        if col.shape[1] == 3:
            col = np.concatenate([col, np.ones((n, 1), np.float32)], 1)
        col = np.ascontiguousarray(col, dtype=np.float32)
        per = self.PAINT_PRIMITIVES[primitive] + 1
        if indices is None:
            idx = self.paint_indices(n, primitive)
        else:
            raw = np.asarray(indices)
            if raw.dtype.kind not in "iu":
                raise ValueError(f"indices must be integers, got {raw.dtype}")
            if raw.size and int(raw.min()) < 0:
                raise ValueError("indices must not be negative")
            idx = np.ascontiguousarray(raw, dtype=np.uint32).ravel()
        if idx.size == 0 or idx.size % per:
            raise ValueError(f"{idx.size} indices do not make {primitive}: their count must be a positive multiple of {per}")
        if idx.size // per > _native.PAINT_MAX_PRIMITIVES:
            raise ValueError(f"a paint call takes at most {_native.PAINT_MAX_PRIMITIVES} primitives, got {idx.size // per}")
        if int(idx.max()) >= n:
            raise ValueError(f"index {int(idx.max())} is out of range: the call has {n} vertices")
        _, half_width, opacity = _stroke(None, width, opacity)
        ids = None
        if features is not None:
            raw = np.asarray(features)
            if raw.shape != (n,) or raw.dtype.kind not in "iu" or (raw.size and int(raw.min()) < 0):
                raise ValueError(f"features must be ({n},) non-negative integers, got shape {raw.shape} of {raw.dtype}")
            ids = np.ascontiguousarray(raw, dtype=np.uint32)
        q = _native.PaintDesc()
        q.struct_size = C.sizeof(_native.PaintDesc)
        q.primitive = self.PAINT_PRIMITIVES[primitive]
        q.vertex_count = n
        q.xz, q.rgba = pts.ctypes.data, col.ctypes.data
        q.feature = ids.ctypes.data if ids is not None else None
        q.indices, q.index_count = idx.ctypes.data, idx.size
        q.half_width, q.opacity = half_width, opacity
        q.aim = self._aim(camera, rearmable)
        self._update(self._lib.f3d_session_paint, q, q.aim.arm, camera)  # (pts, col, ids and idx live until here)

    def _paint_segments(self, entry, q, rgba, width, opacity, camera, rearmable):
        """What paint_contours() and paint_streams() share behind their own arguments: the stroke, the common tail of the two
        descriptors (total, rgba, half_width, opacity, aim), the update.  Returns the number of segments painted."""
        col, half_width, opacity = _stroke(rgba, width, opacity)
        total = C.c_uint64(0)
        q.struct_size = C.sizeof(q)
        q.total = C.addressof(total)
        q.rgba = (C.c_float * 4)(*(float(v) for v in col))
        q.half_width, q.opacity = half_width, opacity
        q.aim = self._aim(camera, rearmable)
        self._update(getattr(self._lib, entry), q, q.aim.arm, camera)  # (what q points to lives in the caller until here)
        return int(total.value)

    def _records_out(self, entry, q, total, out, second):
        """The device form of a call that returns records, ``out=(segments, second)``: the two tensors checked, the capacity and
        the pointers in ``q``, the call, and the views of what was written -- ``segments`` and ``second``'s name their keys."""
        seg, word = out
        if not _is_tensor(seg) or not seg.is_cuda or seg.ndim != 2 or seg.shape[1] != 4 or not seg.is_contiguous() or str(seg.dtype) != "torch.float32":
            raise ValueError(f"out=(segments, {second}): segments must be a contiguous float32 tensor (C, 4) on the session's device")
        if word is not None and (not _is_tensor(word) or not word.is_cuda or word.ndim != 1 or word.shape[0] != seg.shape[0] or
                                 not word.is_contiguous() or str(word.dtype) != "torch.int32"):
            raise ValueError(f"out=(segments, {second}): {second} must be a contiguous int32 tensor (C,) on the session's device, or None")
        q.capacity = int(seg.shape[0])
        q.segments = seg.data_ptr() if seg.shape[0] else None
        setattr(q, second, word.data_ptr() if word is not None and seg.shape[0] else None)
        self._check(getattr(self._lib, entry)(self._handle, C.byref(q), self._err, len(self._err)))
        n = min(int(total.value), int(seg.shape[0]))
        return {"segments": seg[:n], second: None if word is None else word[:n], "total": int(total.value)}

    def _planes(self, q, table, want, out, shape, device_pointers):
        """The planes of a call by name.  ``table``: ``(member of q, NumPy dtype, tensor dtype)`` a plane; ``want``: name -> asked
        for; ``out``: None -- NumPy arrays --, ``"device"`` -- tensors on the session's device -- or a dict of the caller's own
        tensors under the planes' names, checked against ``shape``, the others allocated.  Sets the members of ``q`` (an empty
        plane stays null) and, for tensors, the flag ``device_pointers``; returns name -> plane for the planes of the call."""
        given, device = {}, None
        if out is not None:
            given = {} if isinstance(out, str) else dict(out)
            if (isinstance(out, str) and out != "device") or set(given) - set(want):
                raise ValueError("out must be None, 'device' or a dict of tensors under " + ", ".join(repr(name) for name, _, _ in table))
            device = _form(None, True, None, None, device=f"cuda:{self._device}" if self._device >= 0 else "cuda")
            q.flags |= device_pointers
        got = {}
        for name, dtype, tensor_dtype in table:
            if name in given:
                t = given[name]
                if not _is_tensor(t) or not t.is_cuda or tuple(t.shape) != shape or not t.is_contiguous() or str(t.dtype) != tensor_dtype:
                    raise ValueError(f"out[{name!r}] must be a contiguous {tensor_dtype} tensor ({shape[0]}, {shape[1]}) on the session's device")
            elif want[name]:
                t = _output(device, True, shape, dtype)
            else:
                continue
            got[name] = t
            setattr(q, name, None if shape[0] * shape[1] == 0 else t.ctypes.data if device is None else t.data_ptr())
        return got

    def paint_stats(self):
        """``None`` before the first paint(), else the last call's device times in ms (``count_ms``: count pass and scan,
        ``bin_ms``: emit, sort and run list, ``paint_ms``: the paint kernel) and what it counted (``primitives``, ``keys``: the
        (tile, primitive) pairs, ``tiles``: the non-empty tiles painted).  Waits for the call's kernels."""
        ms, counts = (C.c_double * 3)(), (C.c_uint64 * 3)()
        if not self._lib.f3d_session_paint_stats(self._handle, ms, counts):
            return None
        return {"count_ms": ms[0], "bin_ms": ms[1], "paint_ms": ms[2], "primitives": int(counts[0]), "keys": int(counts[1]), "tiles": int(counts[2])}

    # -- contour lines: extracted, and painted into the drape, on the GPU -------------------------------
    def contour_levels(self, interval, base=0.0):
        """The levels ``base + k * interval`` (float32, ascending) that can cross the session's terrain: over bounds of its
        height range -- heights times the exaggeration, the y of ground() -- kept up by reterrain().  A bound only has to
        contain the range: a level outside it costs a bisection step and draws nothing."""
        interval, base = float(interval), float(base)
        if not np.isfinite(interval) or interval <= 0.0 or not np.isfinite(base):
            raise ValueError(f"interval must be finite and > 0 and base finite, got interval={interval}, base={base}")
        lo, hi = sorted((self._terrain_bottom, self._terrain_top))
        k0, k1 = int(np.floor((lo - base) / interval)), int(np.ceil((hi - base) / interval))
        if k1 - k0 + 1 > _native.CONTOUR_MAX_LEVELS:
            raise ValueError(f"interval {interval} gives {k1 - k0 + 1} levels over heights [{lo}, {hi}]: a call takes at most {_native.CONTOUR_MAX_LEVELS}")
        levels = np.unique((base + np.arange(k0, k1 + 1, dtype=np.float64) * interval).astype(np.float32))
        return levels

    def _contour_levels(self, levels, interval, base):
        if (levels is None) == (interval is None):
            raise ValueError("give either levels or interval=")
        if levels is None:
            return self.contour_levels(interval, base)
        lv = np.ascontiguousarray(np.asarray(levels, dtype=np.float32).reshape(-1))
        if lv.size == 0:
            raise ValueError("levels is empty")
        if lv.size > _native.CONTOUR_MAX_LEVELS:
            raise ValueError(f"a contour call takes at most {_native.CONTOUR_MAX_LEVELS} levels, got {lv.size}")
        if not np.all(np.isfinite(lv)) or not np.all(lv[1:] > lv[:-1]):
            raise ValueError("levels must be finite and strictly ascending (as float32)")
        return lv

    def _cell_region(self, region):
        """``(row0, col0, rows, cols)`` in CELLS, default the whole cell grid.  Whether it lies inside is the library's check."""
        dem_h, dem_w = self.dem_shape
        row0, col0, rows, cols = (0, 0, dem_h - 1, dem_w - 1) if region is None else (int(v) for v in region)
        if min(row0, col0, rows, cols) < 0:
            raise ValueError(f"region=(row0, col0, rows, cols) must not be negative, got {tuple(region)}")
        return row0, col0, rows, cols

    def contours(self, levels=None, *, interval=None, base=0.0, region=None, chain=False, out=None):
        """The contour lines of the terrain this session renders, extracted on the GPU from its own tables (f3d_session_contours):
        marching squares over the cells of ``region`` (``(row0, col0, rows, cols)`` in cells, default all) at ``levels`` --
        finite, strictly ascending float32, in the unit of ground()'s y (heights times the exaggeration) -- or at
        ``base + k * interval`` (contour_levels()).  They stay right after reterrain().
        Returns ``{"segments": (N, 4) float32 (ax, az, bx, bz) in world x-z, "level_index": (N,) uint32 into "levels",
        "levels": the float32 levels, "total": N}``, the segments in block order (8 x 8 blocks of cells row-major, cells row-major
        in a block, levels ascending in a cell).  Ends of neighbouring segments are bit-identical: ``chain=True`` adds
        ``"polylines"`` (chain_contours()).  A level through a DEM sample gives zero-length segments.
        ``out=(segments, level_index)``, torch tensors on the session's device of shape (C, 4) float32 and (C,) int32
        (``level_index`` may be None), takes the device form: the first ``min(N, C)`` records are written there in one call,
        the values returned are views of them and ``"total"`` is N."""
        lv = self._contour_levels(levels, interval, base)
        row0, col0, rows, cols = self._cell_region(region)
        if out is not None and chain:
            raise ValueError("chain=True joins segments on the host: it needs the host form (out=None)")
        total = C.c_uint64(0)
        q = _native.ContoursDesc()
        q.struct_size = C.sizeof(_native.ContoursDesc)
        q.row0, q.col0, q.rows, q.cols = row0, col0, rows, cols
        q.levels, q.level_count = lv.ctypes.data, lv.size
        q.total = C.addressof(total)
        if out is not None:
            q.flags = _native.CONTOUR_DEVICE_POINTERS
            return dict(self._records_out("f3d_session_contours", q, total, out, "level_index"), levels=lv)
        entry = self._lib.f3d_session_contours
        self._check(entry(self._handle, C.byref(q), self._err, len(self._err)))  # (null outputs: the total)
        n = int(total.value)
        seg, idx = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32)
        if n:
            q.capacity = n
            q.segments, q.level_index = seg.ctypes.data, idx.ctypes.data
            self._check(entry(self._handle, C.byref(q), self._err, len(self._err)))
        got = {"segments": seg, "level_index": idx, "levels": lv, "total": n}
        if chain:
            got["polylines"] = self.chain_contours(seg, idx)
        return got

    @staticmethod
    def chain_contours(segments, level_index):
        """Segments of contours() joined into polylines, on the host: ``[{"level_index": k, "closed": bool, "points": (M, 2)
        float32}, ...]`` in order of level, then of the first segment used.  Two segment ends are joined when they belong to
        one level and are bit-identical -- which neighbouring cells' crossings are (a crossing belongs to its lattice edge).  A
        point where exactly two ends meet continues the chain; where more meet (a level through a DEM sample: crossings
        coincide in fours and sixes) or one ends (the region's border), chains end.  A closed loop repeats its first point
        at the end.  Zero-length segments make no chain of their own, but their ends count at the point where they lie."""
        seg = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
        idx = np.asarray(level_index).reshape(-1)
        if idx.shape[0] != seg.shape[0]:
            raise ValueError(f"{seg.shape[0]} segments but {idx.shape[0]} level indices")
        out = []
        seg = np.where(seg == 0.0, np.float32(0.0), seg)  # (-0 and +0 are one point)
        keys = seg.view(np.uint32).reshape(-1, 2, 2).astype(np.uint64)
        keys = (keys[:, :, 0] << np.uint64(32)) | keys[:, :, 1]  # (N, 2): an end's bits
        for level in np.unique(idx):
            rows = np.nonzero((idx == level) & (keys[:, 0] != keys[:, 1]))[0]
            ends = {}
            for r in np.nonzero(idx == level)[0]:  # (a zero-length segment's two ends count where they lie: more than two meet there)
                for e in (0, 1):
                    ends.setdefault(int(keys[r, e]), []).append((int(r), e))
            used = set()

            def walk(r, e):
                """From segment r entered at end e: the points after its first, until a chain end or a return to `r`."""
                pts, first = [], r
                while True:
                    used.add(r)
                    pts.append(seg[r, 2 * (1 - e):2 * (1 - e) + 2])
                    meet = ends[int(keys[r, 1 - e])]
                    if len(meet) != 2:
                        return pts, False
                    (r2, e2) = meet[0] if meet[1] == (r, 1 - e) else meet[1]
                    if r2 == first:
                        return pts, True
                    if r2 in used:
                        return pts, False
                    r, e = r2, e2

            # open chains first, from their ends (points where not exactly two ends meet), then the loops that remain
            for r in rows:
                for e in (0, 1):
                    if int(r) not in used and len(ends[int(keys[r, e])]) != 2:
                        pts, _ = walk(int(r), e)
                        out.append({"level_index": int(level), "closed": False, "points": np.array([seg[r, 2 * e:2 * e + 2]] + pts, np.float32)})
            for r in rows:
                if int(r) not in used:
                    pts, closed = walk(int(r), 0)
                    out.append({"level_index": int(level), "closed": bool(closed), "points": np.array([seg[r, 0:2]] + pts, np.float32)})
        return out

    def paint_contours(self, levels=None, *, interval=None, base=0.0, rgba=(0.0, 0.0, 0.0, 0.8), width=1.0, opacity=1.0, region=None,
                       camera=None, **rearmable):
        """paint() of the terrain's own contour lines, without the segments leaving the GPU (f3d_session_paint_contours): the
        segments contours() returns for ``levels`` (or ``interval`` / ``base``) and ``region`` are emitted into the session's
        paint buffer and rasterised into the drape as ``paint(segments, rgba, primitive="lines", width=width, opacity=opacity)``
        paints them, bit for bit.  One call is one stroke style and one feature (joints blend once); index contours are a
        second call with every n-th level.  ``rgba``: one linear colour with alpha (three numbers: alpha 1).  ``camera`` and the
        other values as reaim() takes them; the render restarts at frame 0; a refused value leaves the session and the canvas
        as they were.  Returns the number of segments painted."""
        self._known("paint_contours", rearmable)
        lv = self._contour_levels(levels, interval, base)
        row0, col0, rows, cols = self._cell_region(region)
        q = _native.PaintContoursDesc()
        q.row0, q.col0, q.rows, q.cols = row0, col0, rows, cols
        q.levels, q.level_count = lv.ctypes.data, lv.size
        return self._paint_segments("f3d_session_paint_contours", q, rgba, width, opacity, camera, rearmable)  # (lv lives until here)

    # -- drainage: flow directions, accumulation, basins, the stream network, on the GPU -------------------
    DRAINAGE_SINK = _native.DRAINAGE_SINK
    # (d_row, d_col) of the direction codes 0 .. 7: E, SE, S, SW, W, NW, N, NE (+col east, +row south); code 8 is a sink
    DRAINAGE_STEPS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))
    _DRAINAGE_PLANES = (("direction", np.uint8, "torch.uint8"), ("accumulation", np.uint32, "torch.int32"), ("basin", np.uint32, "torch.int32"))

    def drainage(self, region=None, *, direction=True, accumulation=True, basin=False, out=None, wait=True):
        """Where water goes over the terrain this session renders, routed on the GPU from its own tables (f3d_session_drainage):
        D8 flow directions -- ``"direction"``, uint8 codes 0 .. 7 = E, SE, S, SW, W, NW, N, NE (DRAINAGE_STEPS), 8 a sink: the
        steepest positive float32 slope, ties to the lowest code; pits, flats and the border's outlets are sinks --, flow
        ``"accumulation"``, uint32: the samples whose path passes through a sample, itself included, and ``"basin"``, uint32: the
        linear index ``row * dem_width + col`` of the sink a sample drains to.  No depressions are filled and no flats
        resolved here: ``session.filled.drainage(...)`` is the same call over the filled surface (fill()), where every path
        reaches the border.  The whole DEM is routed by every call, from the tables as reterrain() left them; ``region``
        (``(row0, col0, rows, cols)`` in samples, default the whole DEM) selects what is returned, as arrays (rows, cols).
        Returns a dict of the planes asked for and always ``"sinks"`` (of the whole DEM), ``"rounds"`` (the path-doubling rounds
        the accumulation took: ``floor(log2(longest)) + 1``) and ``"longest"`` (the longest path, in steps).
        ``out=None`` returns NumPy arrays; ``out="device"``, or a dict of contiguous tensors (rows, cols) on the session's
        device under the planes' names (uint8, int32, int32), takes the device form: nothing crosses the bus but the
        counters.  The call always waits (a counter is read back after every round): ``wait=False`` is refused."""
        if not wait:
            raise ValueError("drainage() always waits: a counter crosses the bus after every doubling round, so there is no wait=False form")
        return self._drainage(region, direction, accumulation, basin, out, False)

    def _drainage(self, region, direction, accumulation, basin, out, fill):
        row0, col0, rows, cols = self._region(region)
        want = {"direction": bool(direction), "accumulation": bool(accumulation), "basin": bool(basin)}
        q = _native.DrainageDesc()
        q.struct_size = C.sizeof(_native.DrainageDesc)
        q.row0, q.col0, q.rows, q.cols = row0, col0, rows, cols
        stats = (C.c_uint32 * 3)()
        q.stats = C.addressof(stats)
        got = self._planes(q, self._DRAINAGE_PLANES, want, out, (rows, cols), _native.DRAINAGE_DEVICE_POINTERS)
        if fill:
            q.flags |= _native.DRAINAGE_FILL
        self._check(self._lib.f3d_session_drainage(self._handle, C.byref(q), self._err, len(self._err)))
        got.update(sinks=int(stats[0]), rounds=int(stats[1]), longest=int(stats[2]))
        return got

    def flow_directions(self, region=None):
        """The D8 direction codes of drainage(), uint8 (rows, cols)."""
        return self.drainage(region, direction=True, accumulation=False)["direction"]

    def flow_accumulation(self, region=None):
        """The flow accumulation of drainage(), uint32 (rows, cols)."""
        return self.drainage(region, direction=False, accumulation=True)["accumulation"]

    def basins(self, region=None):
        """The basin labels of drainage(), uint32 (rows, cols): the linear index of each sample's sink."""
        return self.drainage(region, direction=False, accumulation=False, basin=True)["basin"]

    @staticmethod
    def _threshold(threshold):
        t = int(threshold)
        if t != threshold or not 1 <= t <= 0xFFFFFFFF:
            raise ValueError(f"threshold is an accumulation, an integer from 1 to 2^32 - 1, got {threshold}")
        return t

    STREAMS_FIRST_CAPACITY = 1 << 16  # records the host form of streams() makes room for before it knows the total

    def streams(self, threshold, *, region=None, out=None):
        """The stream network of the terrain (f3d_session_streams): every sample of ``region`` (samples, default the whole DEM)
        that is no sink and has flow accumulation >= ``threshold`` gives one segment from its own lattice point to its
        receiver's (which may lie outside the region), in row-major order of the region's samples.  Returns
        ``{"segments": (N, 4) float32 (ax, az, bx, bz) in world x-z, "accumulation": (N,) uint32, "total": N}``.  The DEM is
        routed by every call (drainage()); the host form makes room for STREAMS_FIRST_CAPACITY records and calls a second
        time only for a larger network.  ``out=(segments, accumulation)``, torch tensors on the session's device of shape
        (C, 4) float32 and (C,) int32 (``accumulation`` may be None), takes the device form: the first ``min(N, C)``
        records are written there in one call, the values returned are views of them and ``"total"`` is N.
        ``session.filled.streams(...)`` is the network over the filled surface."""
        return self._streams(threshold, region, out, False)

    def _streams(self, threshold, region, out, fill):
        t = self._threshold(threshold)
        row0, col0, rows, cols = self._region(region)
        total = C.c_uint64(0)
        q = _native.StreamsDesc()
        q.struct_size = C.sizeof(_native.StreamsDesc)
        q.row0, q.col0, q.rows, q.cols = row0, col0, rows, cols
        q.threshold = t
        q.total = C.addressof(total)
        q.flags = _native.STREAMS_FILL if fill else 0
        if out is not None:
            q.flags |= _native.STREAMS_DEVICE_POINTERS
            return self._records_out("f3d_session_streams", q, total, out, "accumulation")
        room = max(1, min(rows * cols, self.STREAMS_FIRST_CAPACITY))
        while True:
            seg, acc = np.zeros((room, 4), np.float32), np.zeros(room, np.uint32)
            q.capacity = room
            q.segments, q.accumulation = seg.ctypes.data, acc.ctypes.data
            self._check(self._lib.f3d_session_streams(self._handle, C.byref(q), self._err, len(self._err)))
            n = int(total.value)
            if n <= room:
                return {"segments": seg[:n].copy(), "accumulation": acc[:n].copy(), "total": n}
            room = n

    def paint_streams(self, threshold, *, rgba=(0.1, 0.3, 0.8, 1.0), width=1.0, opacity=1.0, region=None, camera=None, fill=False, **rearmable):
        """paint() of the terrain's own stream network, without the segments leaving the GPU (f3d_session_paint_streams): the
        segments streams() returns for ``threshold`` and ``region`` are emitted into the session's paint buffer and rasterised
        into the drape as ``paint(segments, rgba, primitive="lines", width=width, opacity=opacity)`` paints them, bit for bit.
        One call is one stroke style and one feature (confluences blend once); trunk streams are a second call with a
        higher threshold.  ``fill=True`` paints the network over the filled surface (fill()): rivers that cross every lake and
        flat and reach the border.  ``rgba``: one linear colour with alpha (three numbers: alpha 1).  ``camera`` and the other values
        as reaim() takes them; the render restarts at frame 0; a refused value leaves the session and the canvas as they
        were.  Returns the number of segments painted."""
        self._known("paint_streams", rearmable)
        t = self._threshold(threshold)
        row0, col0, rows, cols = self._region(region)
        q = _native.PaintStreamsDesc()
        q.flags = _native.STREAMS_FILL if fill else 0
        q.row0, q.col0, q.rows, q.cols = row0, col0, rows, cols
        q.threshold = t
        return self._paint_segments("f3d_session_paint_streams", q, rgba, width, opacity, camera, rearmable)

    # -- drainage through depressions: the filled surface, and the routing over it ----------------------------
    _FILL_PLANES = (("filled", np.float32, "torch.float32"), ("depth", np.float32, "torch.float32"), ("flat_distance", np.uint32, "torch.int32"))

    def fill(self, region=None, *, filled=True, depth=False, flat_distance=False, out=None):
        """The terrain with its depressions filled to their spill points, computed on the GPU (f3d_session_fill): ``"filled"``,
        float32: the surface W -- the heights on the DEM's border, elsewhere the least height over all paths to the border of
        the highest sample on the path (what priority-flood computes) --, ``"depth"``, float32: ``W - z``, the water depth of
        the lakes, and ``"flat_distance"``, uint32: the steps, within a level stretch of W, to where it drains (0 where a
        neighbour is lower).  ``region`` and ``out`` (None, ``"device"``, or a dict of contiguous tensors (rows, cols) under the
        planes' names: float32, float32, int32) as drainage() takes them.  Returns a dict of the planes asked for and always
        ``"filled_samples"`` (of the whole DEM), ``"fill_rounds"``, ``"flat_rounds"`` (the rounds the two tiled relaxations
        took; they depend on the device's schedule, the planes do not) and ``"largest_flat_distance"``.  The surface is
        computed afresh by every call, from the tables as reterrain() left them."""
        row0, col0, rows, cols = self._region(region)
        want = {"filled": bool(filled), "depth": bool(depth), "flat_distance": bool(flat_distance)}
        q = _native.FillDesc()
        q.struct_size = C.sizeof(_native.FillDesc)
        q.row0, q.col0, q.rows, q.cols = row0, col0, rows, cols
        stats = (C.c_uint32 * 4)()
        q.stats = C.addressof(stats)
        got = self._planes(q, self._FILL_PLANES, want, out, (rows, cols), _native.FILL_DEVICE_POINTERS)
        self._check(self._lib.f3d_session_fill(self._handle, C.byref(q), self._err, len(self._err)))
        got.update(filled_samples=int(stats[0]), fill_rounds=int(stats[1]), flat_rounds=int(stats[2]), largest_flat_distance=int(stats[3]))
        return got

    def filled_heights(self, region=None):
        """The filled surface of fill(), float32 (rows, cols)."""
        return self.fill(region)["filled"]

    def lake_depth(self, region=None):
        """The water depth of fill(), float32 (rows, cols): 0 outside the lakes."""
        return self.fill(region, filled=False, depth=True)["depth"]

    @property
    def filled(self):
        """The drainage calls over the FILLED surface (fill()): ``session.filled.drainage / flow_directions / flow_accumulation /
        basins / streams / paint_streams`` take what the session's own methods take and route with F3D_DRAINAGE_FILL -- water
        leaves every depression over its spill point, crosses every flat, and the only sinks are samples of the border."""
        return FilledRouting(self)

    def drape_image(self, region=None):
        """The session's drape as ``(rows, cols, 3)`` float32 linear RGB -- the values its binary16 texels hold -- after
        everything enqueued on the session, paint() included: what a composed map is saved with.  ``region`` is
        ``(row0, col0, rows, cols)`` in texels, default the whole drape."""
        info = self.drape_info()
        if info is None:
            raise ValueError("this session has no drape to read")
        if region is None:
            reg, rows, cols = None, info["rows"], info["cols"]
        else:
            row0, col0, rows, cols = (int(v) for v in region)
            if min(row0, col0, rows, cols) < 0:
                raise ValueError(f"region=(row0, col0, rows, cols) must not be negative, got {tuple(region)}")
            reg = (C.c_uint32 * 4)(row0, col0, rows, cols)
        out = np.zeros((rows, cols, 3), np.float32)
        self._check(self._lib.f3d_session_drape_read(self._handle, reg, out.ctypes.data, self._err, len(self._err)))
        return out

    # what the four updates share: the keyword check, the camera rule, the call with what the wrapper remembers of it
    def _known(self, method: str, rearmable: dict) -> None:
        unknown = [k for k in rearmable if k not in self.REARMABLE]
        if unknown:
            raise TypeError(f"{method}() got an unexpected keyword argument {unknown[0]!r}")

    def _aim(self, camera, rearmable: dict) -> "_native.ReaimDesc":
        """f3d_session_reaim_desc of an update: ``camera`` as the constructor reads it, or (None) the session's camera and
        current exposure unless ``exposure=`` is given."""
        if camera is None:
            return self._reaim_desc(self._camera, dict(rearmable, exposure=rearmable.get("exposure", self._armed["exposure"])))
        return self._reaim_desc(camera, rearmable)

    def _update(self, entry, desc, arm, camera=None) -> None:
        self._check(entry(self._handle, C.byref(desc), self._err, len(self._err)))
        self._note_armed(arm)
        if camera is not None:
            self._camera = dict(camera)

    def _reaim_desc(self, camera, rearmable: dict) -> "_native.ReaimDesc":
        """f3d_session_reaim_desc of a camera dict and the re-armable values given."""
        a = _native.ReaimDesc()
        a.struct_size = C.sizeof(_native.ReaimDesc)
        a.cam_origin, a.cam_look_at, a.cam_up, a.fov_y_deg, exposure = _native.camera_members(dict(camera))
        given = {k: rearmable.get(k) for k in self.REARMABLE}
        if given["exposure"] is None:
            given["exposure"] = exposure
        a.arm = self._rearm_desc(given)
        return a

    def _rearm_desc(self, given: dict) -> "_native.RearmDesc":
        """f3d_session_rearm_desc of the re-armable values given (None: the session's current one)."""
        values = {k: (self._armed[k] if v is None else v) for k, v in given.items()}
        if given["sun_color"] is not None:
            values["sun_color"] = tuple(_native._extract_sun_color(given["sun_color"]))
        for key in ("seed", "max_frames", "min_frames"):
            if int(values[key]) < 0:
                raise OverflowError("can't convert negative int to unsigned")
        r = _native.RearmDesc()
        r.struct_size = C.sizeof(_native.RearmDesc)
        for key in ("sun_azimuth_deg", "sun_elevation_deg", "sun_intensity", "exposure", "env_intensity", "variance_threshold",
                    "observer_latitude_deg", "observer_longitude_deg", "pressure_mbar", "temperature_c"):
            setattr(r, key, float(values[key]))
        r.sun_color = _native._f3(values["sun_color"])
        r.seed, r.max_frames, r.min_frames = int(values["seed"]), int(values["max_frames"]), int(values["min_frames"])
        return r

    def _note_armed(self, r) -> None:
        # (as the library holds them: float32)
        self._armed = {k: (tuple(float(c) for c in r.sun_color) if k == "sun_color" else type(self._armed[k])(getattr(r, k)))
                       for k in self._armed}

    def render(self) -> dict:
        """The accumulation / convergence loop, resolve and readback of hybrid_render_terrain_reference on this (whole-image)
        session; the same dict, with the frame budget of the create or of the last rearm()."""
        h, w = self.height, self.width
        rgba = np.zeros((h, w, 4), np.uint8)
        alb = np.zeros((h, w, 3), np.float32)
        nrm = np.zeros((h, w, 3), np.float32)
        dep = np.zeros((h, w), np.float32)
        o = _native.Out()
        o.rgba, o.albedo, o.normal, o.depth = rgba.ctypes.data, alb.ctypes.data, nrm.ctypes.data, dep.ctypes.data
        self._check(self._lib.f3d_session_render(self._handle, C.byref(o), self._err, len(self._err)))
        return _native.result_dict(rgba, alb, nrm, dep, o, self._armed["sun_azimuth_deg"], self._armed["sun_elevation_deg"])

    # -- what the query and the four raster families share -----------------------------------
    def _region(self, region):
        """``(row0, col0, rows, cols)``, default the whole DEM.  Whether it lies inside the DEM is the library's check."""
        dem_h, dem_w = self.dem_shape
        row0, col0, rows, cols = (0, 0, dem_h, dem_w) if region is None else (int(v) for v in region)
        if min(row0, col0, rows, cols) < 0:
            raise ValueError(f"region=(row0, col0, rows, cols) must not be negative, got {tuple(region)}")
        return row0, col0, rows, cols

    def _call(self, entry, q, device, wait, region, member, source, outputs):
        """One call of ``entry`` with the descriptor ``q``, whose own members the caller has set: here its size, the flags of
        the form _form() decided (``device``; the same values in every family), the region, the input ``source`` under
        ``member`` and the ``outputs`` (pairs of member name and array or None).  ``source`` is alive until the call returns."""
        q.struct_size = C.sizeof(q)
        if region is not None:
            q.row0, q.col0, q.rows, q.cols = region
        if device is not None:
            q.flags |= _native.RASTER_DEVICE_POINTERS | (0 if wait else _native.RASTER_NO_WAIT)
            if source is not None and source.shape[0]:
                setattr(q, member, source.data_ptr())
            for name, a in outputs:
                if a is not None:
                    setattr(q, name, a.data_ptr())
        else:
            if source is not None and source.shape[0]:
                setattr(q, member, source.ctypes.data)
            for name, a in outputs:
                if a is not None:
                    setattr(q, name, a.ctypes.data)
        self._check(entry(self._handle, C.byref(q), self._err, len(self._err)))

    # -- ray queries: pick, line of sight, ground -----------------------------------------
    GROUND_CLEARANCE = 10.0  # ground() starts its rays this far above the scene's top

    _QUERY_OUTPUTS = {"kind": ((), np.uint32), "t": ((), np.float32), "normal": ((3,), np.float32), "position": ((3,), np.float32),
                      "primitive": ((), np.uint32), "direction": ((3,), np.float32)}  # per ray: shape and dtype of each output member

    def _query(self, mode: int, flags: int, rays, width: int, dtype, outputs, wait: bool = True) -> dict:
        """One f3d_session_query.  ``rays``: a NumPy array (host form: blocking, staged copies through the session's scratch) or
        a torch tensor on the session's device (DEVICE_POINTERS: nothing copied, results are tensors; ``wait=False`` returns
        with the kernel in flight on the session's stream).  ``outputs``: names of f3d_session_query_desc's output members."""
        device = _form(rays, wait, "query", "queries")
        if device is not None:
            if dtype != np.float32 and rays.dtype not in (_torch.int32, _torch.int64, _torch.uint8, _torch.int16):
                raise ValueError("pixels must be an integer tensor")
            if dtype != np.float32 and bool(((rays < 0) | (rays > 0x7FFFFFFF)).any()):
                raise ValueError("pixel coordinates must not be negative")
            r = rays.to(_torch.float32 if dtype == np.float32 else _torch.int32).contiguous()
        else:
            r = np.ascontiguousarray(rays, dtype=dtype)
            if dtype != np.float32 and np.asarray(rays).size and (np.asarray(rays).min() < 0):
                raise ValueError("pixel coordinates must not be negative")
        if r.ndim != 2 or r.shape[1] != width:
            raise ValueError(f"expected shape (N, {width}), got {tuple(np.shape(rays))}")
        n = int(r.shape[0])
        q = _native.QueryDesc()
        q.mode, q.flags, q.count = int(mode), int(flags), n
        out = {name: _output(device, True, (n, *self._QUERY_OUTPUTS[name][0]), self._QUERY_OUTPUTS[name][1]) for name in outputs}
        self._call(self._lib.f3d_session_query, q, device, wait, None, "rays", r, out.items())
        return out

    def trace(self, rays, *, terrain_only: bool = False, wait: bool = True) -> dict:
        """Closest hit of each ray against the scene the session holds NOW (after any reaim / remesh / reterrain, with no
        host wait in between): ``rays`` (N, 8) float32 rows (origin xyz, tmin, direction xyz, tmax), used as given -- ``t`` is
        in units of ``|direction|``.  Returns ``kind`` (0 miss, 1 terrain, 2 mesh), ``t`` (NaN on a miss), ``normal``,
        ``position`` (zeros on a miss) and ``primitive`` (terrain: cx | cz << 16 of the hit cell; mesh: the triangle's row in
        mesh_indices; miss: 0xFFFFFFFF; int32 bits in the tensor form).  ``terrain_only`` leaves the mesh out.  A ray with a
        non-finite component, a zero direction or tmax <= tmin answers as a miss."""
        return self._query(_native.QUERY_CLOSEST, _native.QUERY_TERRAIN_ONLY if terrain_only else 0, rays, 8, np.float32,
                           ("kind", "t", "normal", "position", "primitive"), wait)

    def occluded(self, rays, *, curved: bool = False, terrain_only: bool = False, wait: bool = True):
        """Is anything between tmin and tmax on each ray (the any-hit march of the shadow and IBL rays)?  ``curved``: with the
        sun rays' earth-curvature policy.  Returns a bool array (tensor for a tensor)."""
        flags = (_native.QUERY_CURVED if curved else 0) | (_native.QUERY_TERRAIN_ONLY if terrain_only else 0)
        return self._query(_native.QUERY_OCCLUSION, flags, rays, 8, np.float32, ("kind",), wait)["kind"] != 0

    def pick(self, pixels, *, terrain_only: bool = False, wait: bool = True) -> dict:
        """What the session's current camera sees through the centre of each pixel: ``pixels`` (N, 2) integer rows (x, y) in
        full-image coordinates (a strip session answers for every row).  Returns trace()'s dict plus ``direction``; ``t``
        and ``normal`` are the bits the depth AOV and the G-buffer hold for the pixel."""
        return self._query(_native.QUERY_PIXELS, _native.QUERY_TERRAIN_ONLY if terrain_only else 0, pixels, 2, np.uint32,
                           ("kind", "t", "normal", "position", "primitive", "direction"), wait)

    def ground(self, xz, *, terrain_only: bool = True, top=None):
        """Height of the ground under each (x, z) of ``xz`` (N, 2), float32; NaN outside the DEM's footprint.  Vertical rays
        from ONE height ``top`` (default: GROUND_CLEARANCE above the highest point the session has held), y = top - t:
        every answer carries the rounding of ``top - t`` at the magnitude of ``top``, not of the height.  Measured on the
        CPU oracle (the reference's own arithmetic, not this library): its distance from the f64 bilinear patch is 7.2e-6
        at relief 20 (top 30), about 4 ulp of ``top``; the device returns the oracle's bits.  ``terrain_only=False`` lets a
        mesh triangle above the ground answer (an object then lands on whatever is highest, itself included)."""
        if top is None:
            scene_top = self._terrain_top if (terrain_only or self._mesh_top is None) else max(self._terrain_top, self._mesh_top)
            top = scene_top + self.GROUND_CLEARANCE
        top = float(np.float32(top))
        if _is_tensor(xz):
            import torch

            p = xz.to(torch.float32)
            if p.ndim != 2 or p.shape[1] != 2:
                raise ValueError(f"expected shape (N, 2), got {tuple(xz.shape)}")
            rays = torch.zeros((p.shape[0], 8), dtype=torch.float32, device=p.device)
            rays[:, 0], rays[:, 2] = p[:, 0], p[:, 1]
        else:
            p = np.asarray(xz, dtype=np.float32)
            if p.ndim != 2 or p.shape[1] != 2:
                raise ValueError(f"expected shape (N, 2), got {p.shape}")
            rays = np.zeros((p.shape[0], 8), np.float32)
            rays[:, 0], rays[:, 2] = p[:, 0], p[:, 1]
        rays[:, 1], rays[:, 5], rays[:, 7] = top, -1.0, 1e30
        flags = _native.QUERY_TERRAIN_ONLY if terrain_only else 0
        t = self._query(_native.QUERY_CLOSEST, flags, rays, 8, np.float32, ("t",))["t"]
        return (rays[:, 1] - t) if not isinstance(t, np.ndarray) else (np.float32(top) - t)

    # -- DEM visibility rasters: viewshed, sun mask, sun hours -------------------------------
    SURFACE_BIAS = 1e-3  # rasters start their rays this far above the lifted sample (the shadow rays' own offset)

    def visibility(self, targets, *, toward: bool, curved: bool = False, terrain_only: bool = False, lift: float = 0.0,
                   region=None, masks: bool = True, count: bool = False, wait: bool = True):
        """One f3d_session_raster: from every DEM sample of ``region`` (``(row0, col0, rows, cols)``, default the whole DEM),
        lifted by ``lift``, is each target visible?  ``targets`` (K, 4) float32 rows ``(x, y, z, w)`` ((K, 3): w = 0): with
        ``toward`` a world position and, for ``w > 0``, a maximum horizontal distance; otherwise a direction as given.
        ``None`` (directions only) is the session's current sun.  The device builds the rays from the terrain the session
        holds NOW and marches them as occluded() does (``curved``: with the earth-curvature policy; toward a point the sight
        line drops with it).  A NumPy array takes the host form (blocking), a torch tensor on the session's device the
        device form (results are tensors; ``wait=False`` returns with the kernel in flight on the session's stream, and the
        bits are unpacked on torch's current stream: use it on a session created on that stream).
        Returns the bool array (K, rows, cols) -- True: visible / lit -- for ``masks``, the uint32 array (rows, cols) of the
        number of targets seen for ``count`` (int32 bits as a tensor), ``(masks, count)`` for both."""
        if not (masks or count):
            raise ValueError("visibility() needs an output: masks, count or both")
        region = self._region(region)
        rows, cols = region[2:]
        n = rows * cols
        words = (n + 63) // 64
        q = _native.RasterDesc()
        q.mode = _native.RASTER_TOWARD_POINT if toward else _native.RASTER_ALONG_DIRECTION
        q.flags = (_native.RASTER_CURVED if curved else 0) | (_native.RASTER_TERRAIN_ONLY if terrain_only else 0)
        q.lift = float(lift)
        device = _form(targets, wait, "raster", "rasters")
        if targets is None:
            if toward:
                raise ValueError("targets=None is the session's sun direction: it needs toward=False")
            q.flags |= _native.RASTER_SESSION_SUN
            t, k = None, 1
        else:
            t = _rows4(targets, device)
            k = q.target_count = int(t.shape[0])
        m_out, c_out = _output(device, masks, (k, words), np.uint64), _output(device, count, (n,), np.uint32)
        if device is not None and count and not k:  # (the kernel writes every word of both; without targets nothing runs and nothing is seen)
            c_out.zero_()
        self._call(self._lib.f3d_session_raster, q, device, wait, region, "targets", t, (("masks", m_out), ("count", c_out)))
        out = []
        if masks and device is not None:
            bit = _torch.arange(64, dtype=_torch.int64, device=device)
            out.append((((m_out.unsqueeze(-1) >> bit) & 1) != 0).reshape(k, words * 64)[:, :n].reshape(k, rows, cols))
        elif masks:
            bits = np.unpackbits(m_out.view(np.uint8).reshape(k, words * 8), axis=1, bitorder="little")
            out.append(bits[:, :n].astype(bool).reshape(k, rows, cols))
        if count:
            out.append(c_out.reshape(rows, cols))
        return out[0] if len(out) == 1 else tuple(out)

    def _observers(self, observer, observer_height, max_distance):
        """viewshed()'s observer forms as the float32 (M, 4) rows ``(x, y, z, max_distance or 0)`` of a raster call, and whether
        ONE observer was given: ``(x, z)`` stands ``observer_height`` above ground(), and is dropped without ground under it."""
        obs = np.asarray(observer, dtype=np.float32)
        single = obs.ndim == 1
        obs = np.atleast_2d(obs)
        if obs.ndim != 2 or obs.shape[1] not in (2, 3):
            raise ValueError(f"observer must be (x, y, z), (x, z) or an array of them, got shape {np.asarray(observer).shape}")
        if obs.shape[1] == 2:
            y = self.ground(obs) + np.float32(observer_height)  # (the terrain: an observer does not stand on the mesh)
            obs = np.stack([obs[:, 0], y.astype(np.float32), obs[:, 1]], 1)
            obs = obs[np.isfinite(obs).all(1)]  # (no ground under it: nothing to stand on, nothing seen)
        w = np.float32(0.0 if max_distance is None else max_distance)
        if max_distance is not None and not w > 0.0:
            raise ValueError(f"max_distance must be positive, got {max_distance}")
        return np.concatenate([obs, np.full((len(obs), 1), w, np.float32)], 1).astype(np.float32), single

    def viewshed(self, observer, *, observer_height: float = 1.7, target_height: float = 0.0, max_distance=None,
                 curved: bool = False, terrain_only: bool = False, region=None):
        """Which DEM samples (raised by ``target_height``) does an observer see?  ``observer``: ``(x, y, z)``, an absolute
        position, or ``(x, z)``, standing ``observer_height`` above ground(); an (M, 3) / (M, 2) array of observers gives
        the cumulative viewshed.  ``max_distance``: samples farther away horizontally are not visible.  ``curved``: the
        sight lines follow the session's earth curvature and refraction (one effective radius for the whole DEM).
        Returns the bool array (rows, cols), True: visible, for one observer; for several the uint32 array of how many
        observers see each sample.  An observer outside the DEM's footprint given as ``(x, z)`` sees nothing."""
        targets, single = self._observers(observer, observer_height, max_distance)
        lift = np.float32(np.float32(target_height) + np.float32(self.SURFACE_BIAS))
        if single:
            if len(targets) == 0:  # (no target is a checked no-op of the library: the region is validated, nothing is seen)
                return self.visibility(targets, toward=True, curved=curved, terrain_only=terrain_only, lift=lift, region=region,
                                       masks=False, count=True) != 0
            return self.visibility(targets, toward=True, curved=curved, terrain_only=terrain_only, lift=lift, region=region)[0]
        return self.visibility(targets, toward=True, curved=curved, terrain_only=terrain_only, lift=lift, region=region,
                               masks=False, count=True)

    def shadow_mask(self, direction=None, *, curved: bool = True, terrain_only: bool = False, region=None):
        """Which DEM samples are lit from ``direction`` (toward the light; None: the session's current sun, as the frames'
        sun rays use it)?  Returns the bool array (rows, cols), True: lit, as the reference's shadow_mask."""
        targets = None if direction is None else np.asarray(direction, dtype=np.float32).reshape(1, 3)
        return self.visibility(targets, toward=False, curved=curved, terrain_only=terrain_only, lift=np.float32(self.SURFACE_BIAS),
                               region=region)[0]

    def sun_hours(self, directions, *, curved: bool = True, terrain_only: bool = False, region=None):
        """From how many of ``directions`` (N, 3) is each DEM sample lit?  Returns the uint32 array (rows, cols).  A direction
        with ``y <= 0`` (the sun below the horizontal) is dropped here and lights nothing."""
        d = np.asarray(directions, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError(f"expected shape (N, 3), got {d.shape}")
        d = d[d[:, 1] > 0.0]
        return self.visibility(d, toward=False, curved=curved, terrain_only=terrain_only, lift=np.float32(self.SURFACE_BIAS),
                               region=region, masks=False, count=True)

    # -- horizon rasters: horizon slopes, sky-view factor -----------------------------------
    @staticmethod
    def horizon_directions(azimuths=16):
        """The float32 (K, 2) rows ``(dx, dz)`` a horizon() / sky_view_factor() call with these ``azimuths`` uses.  An int N:
        the compass headings ``360 k / N`` degrees, k = 0 .. N - 1, in the convention of ``sun_azimuth_deg`` -- ``(dx, dz) =
        (sin a, -cos a)``, computed in float64 and rounded to float32 (0 is north, -z; 90 east, +x).  A (K, 2) array is used as
        given; a torch tensor stays a tensor.  ``(dx_k, s, dz_k)`` is then the direction whose visibility ``s > H_k`` answers."""
        if isinstance(azimuths, (int, np.integer)) and not isinstance(azimuths, bool):
            n = int(azimuths)
            if not 1 <= n <= _native.HORIZON_MAX_AZIMUTHS:
                raise ValueError(f"azimuths must be 1 to {_native.HORIZON_MAX_AZIMUTHS}, got {n}")
            a = np.radians(360.0 * np.arange(n, dtype=np.float64) / n)
            return np.stack([np.sin(a), -np.cos(a)], 1).astype(np.float32)
        if _is_tensor(azimuths):
            import torch

            d = azimuths.to(torch.float32)
            if d.ndim != 2 or d.shape[1] != 2:
                raise ValueError(f"expected shape (K, 2), got {tuple(azimuths.shape)}")
            return d.contiguous()
        d = np.ascontiguousarray(azimuths, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] != 2:
            raise ValueError(f"expected shape (K, 2), got {d.shape}")
        return d

    def _horizon(self, azimuths, lift, curved, region, planes, sky_view, wait):
        region = self._region(region)
        rows, cols = region[2:]
        d = self.horizon_directions(azimuths)
        k = int(d.shape[0])
        q = _native.HorizonDesc()
        q.flags = _native.HORIZON_CURVED if curved else 0
        q.lift = float(lift)
        q.azimuth_count = k
        device = _form(d, wait, "horizon", "horizons")
        h_out, s_out = _output(device, planes, (k, rows, cols), np.float32), _output(device, sky_view, (rows, cols), np.float32)
        self._call(self._lib.f3d_session_horizon, q, device, wait, region, "azimuths", d, (("horizon", h_out), ("sky_view", s_out)))
        return h_out, s_out

    def horizon(self, azimuths=16, *, lift: float = SURFACE_BIAS, curved: bool = False, region=None, sky_view: bool = False,
                wait: bool = True):
        """One f3d_session_horizon: for every DEM sample of ``region`` (``(row0, col0, rows, cols)``, default the whole DEM),
        lifted by ``lift`` >= 0, and every azimuth, the slope ``H`` under which the ground hides the sky along that azimuth --
        the supremum of ``(y - k t^2 - o.y) / t`` over the terrain ahead (terrain only: a mesh is not a horizon), -inf where no
        terrain lies ahead.  ``azimuths``: see horizon_directions().  ``(dx, H, dz)`` is the grazing direction of visibility()
        along a direction with the same ``curved``; for unit ``(dx, dz)`` H is the tangent of the horizon's elevation.  A
        NumPy array or an int takes the host form (blocking); a torch tensor on the session's device the device form (results
        are tensors; ``wait=False`` returns with the kernel in flight on the session's stream).
        Returns the float32 array (K, rows, cols), and ``(horizon, sky_view)`` with ``sky_view=True``."""
        h, s = self._horizon(azimuths, lift, curved, region, True, sky_view, wait)
        return (h, s) if sky_view else h

    def sky_view_factor(self, azimuths=16, *, lift: float = SURFACE_BIAS, curved: bool = False, region=None, wait: bool = True):
        """The horizontal-surface sky-view factor (Dozier-Frew / Zaksek) of every DEM sample of ``region``: ``1 - mean_k
        sin(elevation of horizon k)``, horizons below the horizontal counting 0.  float32 (rows, cols); the K horizon planes
        are never materialised, on the device or here.  Arguments as horizon()."""
        return self._horizon(azimuths, lift, curved, region, False, True, wait)[1]

    # -- clearance rasters: the height needed to be seen --------------------------------------
    def clearance(self, observers, *, curved: bool = False, region=None, planes: bool = True, lowest: bool = False, wait: bool = True):
        """One f3d_session_clearance: for every DEM sample of ``region`` (``(row0, col0, rows, cols)``, default the whole DEM)
        and every observer, how far above the ground a target over the sample must stand for the observer to see it -- the
        smallest ``lift`` at which ``visibility(observer, toward=True, lift=lift, terrain_only=True)`` answers True, as an
        exact max-slope walk of the session's min/max pyramid (terrain only: a mesh hides nothing here).  ``observers``
        (K, 4) float32 rows ``(x, y, z, w)`` ((K, 3): w = 0): a world position and, for ``w > 0``, a maximum horizontal
        distance.  0: the ground itself shows; +inf: out of range, or the observer lies under the surface; NaN: a non-finite
        observer handed in as a tensor.  ``curved``: the sight lines follow the session's earth curvature, as visibility()'s.
        A NumPy array takes the host form (blocking); a torch tensor on the session's device the device form (results are
        tensors; ``wait=False`` returns with the kernel in flight on the session's stream).
        Returns the float32 array (K, rows, cols) for ``planes``, the float32 array (rows, cols) of the minimum over the
        observers ("seen by any of them"; the K planes are then never materialised) for ``lowest``, ``(planes, lowest)`` for
        both.  ``viewshed(obs, target_height=th) == (visible_height(obs) < th + SURFACE_BIAS)`` away from a band of rounding
        around the threshold."""
        if not (planes or lowest):
            raise ValueError("clearance() needs an output: planes, lowest or both")
        region = self._region(region)
        rows, cols = region[2:]
        device = _form(observers, wait, "clearance", "clearances")
        t = _rows4(observers, device)
        k = int(t.shape[0])
        q = _native.ClearanceDesc()
        q.flags = _native.CLEARANCE_CURVED if curved else 0
        q.observer_count = k
        h_out, l_out = _output(device, planes, (k, rows, cols), np.float32), _output(device, lowest, (rows, cols), np.float32)
        self._call(self._lib.f3d_session_clearance, q, device, wait, region, "observers", t, (("height", h_out), ("lowest", l_out)))
        return (h_out, l_out) if (planes and lowest) else (h_out if planes else l_out)

    def visible_height(self, observer, *, observer_height: float = 1.7, max_distance=None, curved: bool = False, region=None):
        """How high above the ground must a target over each DEM sample stand to be seen by at least one observer?  The
        "above ground level" raster of a GIS viewshed: one pass is viewshed() for every ``target_height`` at once.
        ``observer``: viewshed()'s forms -- ``(x, y, z)``, an absolute position, or ``(x, z)``, standing ``observer_height``
        above ground(), or an (M, 3) / (M, 2) array of them.  ``max_distance``: samples farther away horizontally are never
        seen.  Returns the float32 array (rows, cols): 0 where the ground itself shows, +inf where the sample is out of
        range or no observer has ground under it (then every sample is +inf, as viewshed() sees nothing).
        ``viewshed(obs, target_height=th) == (visible_height(obs) < th + SURFACE_BIAS)`` away from a band of rounding around
        the threshold (terrain only: a mesh hides nothing here)."""
        observers, _ = self._observers(observer, observer_height, max_distance)
        if len(observers) == 0:
            dem_h, dem_w = self.dem_shape
            row0, col0, rows, cols = (0, 0, dem_h, dem_w) if region is None else (int(v) for v in region)
            if min(row0, col0) < 0 or min(rows, cols) <= 0 or row0 + rows > dem_h or col0 + cols > dem_w:
                raise ValueError(f"region=(row0, col0, rows, cols)={tuple(region)} is empty or reaches outside the {dem_h}x{dem_w} DEM")
            return np.full((rows, cols), np.inf, np.float32)
        return self.clearance(observers, curved=curved, region=region, planes=False, lowest=True)

    # -- shadow-depth rasters: the height needed to be lit --------------------------------------
    def umbra(self, directions=None, *, curved: bool = True, region=None, planes: bool = True, deepest: bool = False, wait: bool = True):
        """One f3d_session_umbra: for every DEM sample of ``region`` (``(row0, col0, rows, cols)``, default the whole DEM) and
        every direction, how far above the ground a point over the sample must stand to be lit from that direction -- the
        smallest ``lift`` at which ``visibility(direction, toward=False, lift=lift, terrain_only=True)`` answers True, as one
        bounded walk of the session's min/max pyramid (terrain only: a mesh casts no shadow here).  ``directions`` (K, 4)
        float32 rows ``(dx, dy, dz, 0)`` ((K, 3): the fourth is 0), toward the light, used as given; ``None`` is the session's
        current sun, as the frames' sun rays use it.  0: the ground itself is lit; +inf: straight down; NaN: a non-finite or
        zero direction handed in as a tensor.  ``dy <= 0`` is legal (the DEM's footprint is finite).  ``curved``: the rays follow
        the session's earth curvature, as shadow_mask()'s.  A NumPy array (or None) takes the host form (blocking); a torch
        tensor on the session's device the device form (results are tensors; ``wait=False`` returns with the kernel in flight
        on the session's stream).
        Returns the float32 array (K, rows, cols) for ``planes``, the float32 array (rows, cols) of the maximum over the
        directions ("lit from all of them above this"; the K planes are then never materialised) for ``deepest``,
        ``(planes, deepest)`` for both.  ``shadow_mask(d) == (lit_height(d) < SURFACE_BIAS)`` away from a band of rounding
        around the threshold."""
        if not (planes or deepest):
            raise ValueError("umbra() needs an output: planes, deepest or both")
        region = self._region(region)
        rows, cols = region[2:]
        device = _form(directions, wait, "umbra", "umbras")
        q = _native.UmbraDesc()
        q.flags = _native.UMBRA_CURVED if curved else 0
        if directions is None:
            q.flags |= _native.UMBRA_SESSION_SUN
            t, k = None, 1
        else:
            t = _rows4(directions, device)
            k = q.direction_count = int(t.shape[0])
        p_out, d_out = _output(device, planes, (k, rows, cols), np.float32), _output(device, deepest, (rows, cols), np.float32)
        self._call(self._lib.f3d_session_umbra, q, device, wait, region, "directions", t, (("depth", p_out), ("deepest", d_out)))
        return (p_out, d_out) if (planes and deepest) else (p_out if planes else d_out)

    def lit_height(self, direction=None, *, curved: bool = True, region=None):
        """How high above the ground must a point over each DEM sample stand to be lit?  ``direction``: one ``(x, y, z)`` toward
        the light (None: the session's current sun), or a track (N, 3): then the height above which the sample is lit from
        EVERY position of the track.  A position with ``y <= 0`` (the sun below the horizontal) is dropped, as sun_hours()
        drops it; an empty track returns zeros.  Returns the float32 array (rows, cols): 0 where the ground itself is lit.
        ``shadow_mask(d) == (lit_height(d) < SURFACE_BIAS)`` away from a band of rounding around the threshold (terrain only:
        a mesh casts no shadow here)."""
        if direction is None:
            return self.umbra(None, curved=curved, region=region)[0]
        d = np.asarray(direction, dtype=np.float32)
        if d.ndim == 1:
            d = d.reshape(1, -1)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError(f"expected a direction (x, y, z) or a track of shape (N, 3), got {np.asarray(direction).shape}")
        d = d[d[:, 1] > 0.0]
        if len(d) == 0:
            row0, col0, rows, cols = self._region(region)
            dem_h, dem_w = self.dem_shape
            if min(rows, cols) <= 0 or row0 + rows > dem_h or col0 + cols > dem_w:
                raise ValueError(f"region=(row0, col0, rows, cols)={tuple(region)} is empty or reaches outside the {dem_h}x{dem_w} DEM")
            return np.zeros((rows, cols), np.float32)
        return self.umbra(d, curved=curved, region=region, planes=False, deepest=True)

    # -- irradiation rasters: beam energy over a sun track, surface normals --------------------
    @staticmethod
    def irradiation_terms(directions, weights=None):
        """The (K, 4) float32 rows ``(x, y, z, weight)`` an irradiation() call with these arguments sends: ``directions`` (K, 3)
        with ``weights`` (K,), or (K, 4) with the weight in the last column (``weights`` must then be None); a direction with
        ``y <= 0`` -- the sun below the horizontal -- gets weight 0.  A torch tensor stays a tensor."""
        tensors = _is_tensor(directions)
        if tensors:
            import torch

            d = directions.to(torch.float32)
        else:
            d = np.asarray(directions, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] not in (3, 4):
            raise ValueError(f"expected directions of shape (K, 3) or (K, 4), got {tuple(d.shape)}")
        if d.shape[1] == 4:
            if weights is not None:
                raise ValueError("(K, 4) directions carry their weights: weights must be None")
            xyz, w = d[:, :3], d[:, 3]
        else:
            if weights is None:
                raise ValueError("(K, 3) directions need weights (K,)")
            if tensors:
                w = torch.as_tensor(weights, dtype=torch.float32, device=d.device).reshape(-1)
            else:
                w = np.asarray(weights, dtype=np.float32).reshape(-1)
            if w.shape[0] != d.shape[0]:
                raise ValueError(f"{d.shape[0]} directions but {w.shape[0]} weights")
            xyz = d
        if tensors:
            w = torch.where(xyz[:, 1] > 0.0, w, torch.zeros_like(w))
            return torch.cat([xyz, w[:, None]], 1).contiguous()
        w = np.where(xyz[:, 1] > 0.0, w, np.float32(0.0)).astype(np.float32)
        return np.ascontiguousarray(np.concatenate([xyz, w[:, None]], 1), dtype=np.float32)

    def _irradiation(self, terms, flags, lift, region, energy, count, normal, wait, device=None):
        region = self._region(region)
        rows, cols = region[2:]
        q = _native.IrradiationDesc()
        q.flags = flags
        q.lift = float(lift)
        q.direction_count = 0 if terms is None else int(terms.shape[0])
        device = _form(terms, wait, "irradiation", "irradiations", device)
        e_out, c_out = _output(device, energy, (rows, cols), np.float32), _output(device, count, (rows, cols), np.uint32)
        n_out = _output(device, normal, (rows, cols, 3), np.float32)
        self._call(self._lib.f3d_session_irradiation, q, device, wait, region, "directions", terms,
                   (("energy", e_out), ("count", c_out), ("normal", n_out)))
        return e_out, c_out, n_out

    def irradiation(self, directions, weights=None, *, horizontal: bool = False, curved: bool = True, terrain_only: bool = False,
                    lift: float = SURFACE_BIAS, region=None, count: bool = False, wait: bool = True):
        """One f3d_session_irradiation: for every DEM sample of ``region`` (``(row0, col0, rows, cols)``, default the whole DEM)
        the energy the direct beam delivers over the sun positions ``directions`` (toward the sun; (K, 3) with ``weights``
        (K,), or (K, 4) with the weight in the last column; they need not be unit): the sum over the positions of ``weight x
        cos(incidence on the local slope)`` wherever that cosine is positive and the shadow ray -- the one shadow_mask()
        marches, from the sample lifted by ``lift``, under ``curved`` / ``terrain_only`` -- is unblocked.  Weights in W/m^2 x
        hours give Wh/m^2.  A facet that faces away from a position marches no ray for it.  A direction with ``y <= 0`` (the
        sun below the horizontal) gets weight 0 here, as sun_hours() drops it.  ``horizontal``: the beam on a horizontal plane
        (the cosine is the sine of the sun's elevation) instead of the slope.  The slope is surface_normals()'s.  A NumPy
        array takes the host form (blocking); a torch tensor on the session's device the device form (results are tensors;
        ``wait=False`` returns with the kernel in flight on the session's stream).
        Returns the float32 array (rows, cols), or ``(energy, count)`` with ``count=True``: the uint32 array (int32 bits as a
        tensor) of the number of positions that contributed."""
        terms = self.irradiation_terms(directions, weights)
        flags = ((_native.IRRADIATION_HORIZONTAL if horizontal else 0) | (_native.IRRADIATION_CURVED if curved else 0)
                 | (_native.IRRADIATION_TERRAIN_ONLY if terrain_only else 0))
        e, c, _ = self._irradiation(terms, flags, lift, region, True, count, False, wait)
        return (e, c) if count else e

    def surface_normals(self, region=None, wait: bool = True):
        """The unit surface normals irradiation() takes its cosines against, float32 (rows, cols, 3) as ``(x, y, z)`` with y up:
        ``(-gx, 1, -gz) / sqrt(gx^2 + gz^2 + 1)`` where ``(gx, gz)`` is the central difference (one-sided on the DEM's border) of
        the heights the session holds NOW -- exaggeration applied, reterrain() followed -- over the sample spacing.  Slope and
        aspect follow from them: the slope angle is ``arccos(n_y)`` (its tangent ``hypot(n_x, n_z) / n_y``), and the aspect --
        the compass heading the facet faces, downhill, in the convention of ``sun_azimuth_deg`` (0 north = -z, 90 east = +x) --
        is ``atan2(n_x, -n_z)``, undefined where the slope is 0.  No ray is marched.  Returns a NumPy array (host form,
        blocking); with ``wait=False`` a torch tensor on the session's device, the kernel in flight on the session's stream."""
        device = None
        if not wait:
            import torch

            device = torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())
        return self._irradiation(None, 0, 0.0, region, False, False, True, wait, device)[2]

    def insolation(self, track, *, dni=None, dhi=None, azimuths=16, **irradiation_kwargs) -> dict:
        """A solar-exposure map over a sun track (``insolation.sun_track``: ``directions``, ``elevation_deg``, ``hours``), in
        Wh/m^2, float32 (rows, cols) each:

        * ``direct``   ``irradiation(track directions, dni x hours)``: the beam on the local slope, shadows cast;
        * ``diffuse``  ``sky_view_factor(azimuths) x sum(dhi x hours)``: an ISOTROPIC sky seen through the horizontal-surface
          sky-view factor -- an approximation: the sky is brighter near the sun and the horizon, and a steep facet sees less
          sky, and some ground, which this ignores;
        * ``global``   their sum.

        ``dni`` / ``dhi`` (W/m^2, (K,)) default to ``insolation.clear_sky`` of the track's elevations; measured values go in
        instead.  ``irradiation_kwargs`` (horizontal, curved, terrain_only, lift, region) go to irradiation(); ``curved``,
        ``lift`` and ``region`` to sky_view_factor() as well.  Host form."""
        from . import insolation as _insolation

        unknown = set(irradiation_kwargs) - {"horizontal", "curved", "terrain_only", "lift", "region"}
        if unknown:
            raise TypeError(f"insolation() got unexpected keyword arguments {sorted(unknown)}")
        hours = np.asarray(track["hours"], np.float64)
        if dni is None or dhi is None:
            clear = _insolation.clear_sky(track["elevation_deg"])
            dni = clear[0] if dni is None else dni
            dhi = clear[1] if dhi is None else dhi
        dni, dhi = np.asarray(dni, np.float64), np.asarray(dhi, np.float64)
        direct = self.irradiation(np.asarray(track["directions"], np.float32), (dni * hours).astype(np.float32), **irradiation_kwargs)
        sky = {k: v for k, v in irradiation_kwargs.items() if k in ("curved", "lift", "region")}
        diffuse = (self.sky_view_factor(azimuths, **sky) * np.float32((dhi * hours).sum())).astype(np.float32)
        return {"direct": direct, "diffuse": diffuse, "global": (direct + diffuse).astype(np.float32)}

    def certificates(self) -> dict:
        """Diagnostics (synchronises): content hashes of the sun-ray and primary-ray certificates."""
        out = (C.c_uint64 * 2)()
        if self._lib.f3d_session_certificates(self._handle, out) != 0:
            raise RuntimeError("f3d_session_certificates failed")
        return {"sun_clear": int(out[0]), "primary_start": int(out[1])}

    def sky_blocks(self) -> dict:
        """Diagnostics (synchronises): the session's deep-sky blocks -- 8 x 8 pixel blocks so far inside certified sky that
        a frame only accumulates there.  0 deep blocks for a session whose frames use no such table."""
        out = (C.c_uint32 * 4)()
        if self._lib.f3d_session_sky_blocks(self._handle, out) != 0:
            raise RuntimeError("f3d_session_sky_blocks failed")
        return {"blocks": int(out[0]), "deep_blocks": int(out[1]), "certified_pixels": int(out[2]), "deep_pixels": int(out[3])}

    # -- stepping ---------------------------------------------------------------------
    def enqueue_frames(self, first_frame: int, count: int, collect_stats: bool = False):
        """Asynchronously enqueue accumulation frames on the session stream."""
        self._check(self._lib.f3d_session_enqueue_frames(self._handle, int(first_frame), int(count),
                                                         1 if collect_stats else 0, self._err, len(self._err)))

    def enqueue_trace(self, first_frame: int, count: int):
        """Frames in flight: trace frames [first_frame, first_frame + count) in one launch (count <= frames_in_flight())."""
        self._check(self._lib.f3d_session_enqueue_trace(self._handle, int(first_frame), int(count), self._err, len(self._err)))

    def enqueue_merge(self, frame: int, collect_stats: bool = False):
        """Frames in flight: the ordered half (reservoir chain, accumulation) of one traced frame."""
        self._check(self._lib.f3d_session_enqueue_merge(self._handle, int(frame), 1 if collect_stats else 0, self._err, len(self._err)))

    def frames_in_flight(self) -> int:
        """Effective number of frames the session traces per launch (0: every frame is one fused launch)."""
        return int(self._lib.f3d_session_frames_in_flight(self._handle))

    def trace_batch(self, frame: int, remaining: int) -> int:
        """Batch size to trace next at `frame` (short batches first, then frames_in_flight())."""
        return int(self._lib.f3d_session_trace_batch(self._handle, int(frame), int(remaining)))

    def retraced_pixels(self) -> int:
        """Diagnostics (synchronises): pixel-frames whose sun-direction prediction failed and were traced again."""
        total = C.c_uint64(0)
        self._lib.f3d_session_retraced_pixels(self._handle, C.byref(total))
        return int(total.value)

    FINGERPRINT_FIELDS = ("camera", "light", "terrain_scalars", "mesh_scalars", "scalars", "leaf_table", "band_tables",
                          "mesh_vertices", "mesh_indices", "bvh_nodes", "bvh_triangles", "environment", "gbuffer",
                          "reservoirs", "accumulation", "frame_heads", "drape")

    def fingerprint(self) -> dict:
        """Diagnostics (synchronises): hashes of everything a frame launch reads, by name."""
        out = (C.c_uint64 * 17)()
        if self._lib.f3d_session_fingerprint(self._handle, out, 17) != 0:
            raise RuntimeError("f3d_session_fingerprint failed")
        return dict(zip(self.FINGERPRINT_FIELDS, (int(v) for v in out)))

    # records of f3d_session_mesh_tree (f3d_scene.h BvhNode / Bvh4Node; a triangle corner: xyz and the bits of w)
    BVH_NODE = np.dtype([("bmin", "<f4", 3), ("skip", "<u4"), ("bmax", "<f4", 3), ("leaf", "<u4")])
    BVH4_NODE = np.dtype([("lo_x", "<f4", 4), ("hi_x", "<f4", 4), ("lo_y", "<f4", 4), ("hi_y", "<f4", 4), ("lo_z", "<f4", 4),
                          ("hi_z", "<f4", 4), ("leaf", "<u4", 4), ("first_child", "<u4"), ("inner", "<u4"), ("pad", "<u4", 2)])
    BVH_CORNER = np.dtype([("xyz", "<f4", 3), ("w", "<u4")])

    def mesh_tree(self):
        """Diagnostics (synchronises): ``(form, nodes, tris)`` -- the mesh BVH the frame launches walk, read back from the
        device as it is now (after a remesh() refit: the session's own tree).  ``form`` 0: no tree (empty arrays), 1: ``nodes``
        are BVH_NODE records in threaded preorder, 2: BVH4_NODE records; ``tris`` has shape (triangles, 3) of BVH_CORNER in
        leaf order, the original triangle index in ``tris["w"][:, 0]``."""
        info = (C.c_uint32 * 4)()
        self._check(self._lib.f3d_session_mesh_tree(self._handle, info, None, 0, None, 0, self._err, len(self._err)))
        form, node_count, tri_count = int(info[0]), int(info[1]), int(info[2])
        nodes = np.zeros(node_count, self.BVH4_NODE if form == 2 else self.BVH_NODE)
        tris = np.zeros((tri_count, 3), self.BVH_CORNER)
        self._check(self._lib.f3d_session_mesh_tree(self._handle, info, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes,
                                                    self._err, len(self._err)))
        if (int(info[0]), int(info[1]), int(info[2])) != (form, node_count, tri_count):
            raise RuntimeError("f3d_session_mesh_tree: the tree changed between the two calls")
        return form, nodes, tris

    def enqueue_frame_part(self, frame: int, part: int, collect_stats: bool = False):
        """One frame in two launches: part 1 = head + the strip's edge rows (the halo donors), part 2 = interior."""
        self._check(self._lib.f3d_session_enqueue_frame_part(self._handle, int(frame), int(part),
                                                             1 if collect_stats else 0, self._err, len(self._err)))

    # -- peer halos (strips of one node without the host or a collective in the frame chain) -------------
    def halo_export(self) -> bytes:
        """What a neighbouring strip needs to map this strip's reservoirs and its frame counter (f3d_halo_export bytes)."""
        rec = _native.HaloExport()
        self._check(self._lib.f3d_session_halo_export(self._handle, C.byref(rec), self._err, len(self._err)))
        return bytes(rec)

    def halo_connect(self, side: int, export: bytes):
        """side 0: the strip above (smaller rows), 1: the strip below; export = that strip's halo_export()."""
        rec = _native.HaloExport.from_buffer_copy(export)
        self._check(self._lib.f3d_session_halo_connect(self._handle, int(side), C.byref(rec), self._err, len(self._err)))

    def halo_probe_publish(self, nonce: int):
        """Link check, step 1: store `nonce` into this strip's counter block (the store the frame counter uses)."""
        self._check(self._lib.f3d_session_halo_probe(self._handle, 0, int(nonce) & 0xFFFFFFFF, None, self._err, len(self._err)))

    def halo_probe_read(self):
        """Link check, step 2 (after a barrier): the neighbours' words as this device reads them: (above, below)."""
        seen = (C.c_uint32 * 2)()
        self._check(self._lib.f3d_session_halo_probe(self._handle, 1, 0, seen, self._err, len(self._err)))
        return int(seen[0]), int(seen[1])

    def halo_probe_fill(self, nonce: int):
        """Link check with a real block, step 1: fill this strip's two edge blocks of reservoir buffer 0 with the pattern of
        `nonce` (a many-workgroup kernel, as the frame kernels leave their rows) and publish the nonce behind it."""
        self._check(self._lib.f3d_session_halo_probe(self._handle, 2, int(nonce) & 0xFFFFFFFF, None, self._err, len(self._err)))

    def halo_probe_pull(self, nonce_above: int, nonce_below: int):
        """Step 2: wait (on the device) for the neighbours' nonces, pull their blocks with the frame loop's kernel and compare
        the sums with the patterns'; raises if a block is not what its owner wrote."""
        seen = (C.c_uint32 * 2)(int(nonce_above) & 0xFFFFFFFF, int(nonce_below) & 0xFFFFFFFF)
        self._check(self._lib.f3d_session_halo_probe(self._handle, 3, 0, seen, self._err, len(self._err)))
        return int(seen[0]), int(seen[1])

    def halo_probe_clear(self):
        """Step 3, once EVERY strip has pulled (a barrier): reservoir buffer 0 as a new session has it."""
        self._check(self._lib.f3d_session_halo_probe(self._handle, 4, 0, None, self._err, len(self._err)))

    def halo_timeouts(self) -> int:
        """Device-side halo waits of the last enqueue_batch_strip that gave up (a neighbour that stopped); synchronises."""
        n = C.c_uint32(0)
        self._check(self._lib.f3d_session_halo_status(self._handle, C.byref(n), self._err, len(self._err)))
        return int(n.value)

    def halo_stats(self, reset: bool = False) -> dict:
        """How long this strip's pulls stood waiting for its neighbours (device time, ms) since the last reset; synchronises."""
        rec = _native.HaloStats()
        rec.reset = 1 if reset else 0
        self._check(self._lib.f3d_session_halo_stats(self._handle, C.byref(rec), self._err, len(self._err)))
        return {"frames_published": int(rec.frames_published), "timeouts": int(rec.timeouts), "pulls": int(rec.pulls),
                "wait_ms": (float(rec.wait_ms[0]), float(rec.wait_ms[1])), "longest_wait_ms": float(rec.longest_wait_ms),
                "timeout_ms": float(rec.timeout_ms)}

    def enqueue_batch_strip(self, first_frame: int, count: int, collect_stats: bool = False):
        """Frames [first_frame, first_frame + count) of a connected strip in ONE call: per frame its kernels, the frame
        counter, the pull of both neighbours' edge rows -- no host synchronisation, no collective."""
        self._check(self._lib.f3d_session_enqueue_batch_strip(self._handle, int(first_frame), int(count), 1 if collect_stats else 0,
                                                              self._err, len(self._err)))

    def window_stats(self):
        """(max Welford m2 over the owned pixels, saw non-finite) -- synchronises the stream."""
        m2, bad = C.c_float(0.0), C.c_int32(0)
        self._check(self._lib.f3d_session_window_stats(self._handle, C.byref(m2), C.byref(bad), self._err,
                                                       len(self._err)))
        return float(m2.value), bool(bad.value)

    def halo(self, which: int, side: int):
        """(device pointer, bytes) of a halo block (HALO_ROWS rows) of reservoir buffer `which`."""
        ptr, nbytes = C.c_void_p(None), C.c_uint64(0)
        rc = self._lib.f3d_session_halo(self._handle, int(which), int(side), C.byref(ptr), C.byref(nbytes))
        if rc != 0:
            raise ValueError("invalid halo query")
        return int(ptr.value), int(nbytes.value)

    def set_accumulation(self, sums_rgba):
        """Replace the accumulated radiance sums by (rows, width, 4) f32 sums of the caller's (composition hook: the PBR
        tracer's radiance through this session's resolve and AETHER post)."""
        arr = np.ascontiguousarray(sums_rgba, np.float32)
        if arr.shape != (self.rows, self.width, 4):
            raise ValueError(f"accumulation must have shape ({self.rows}, {self.width}, 4)")
        self._check(self._lib.f3d_session_set_accumulation(self._handle, arr.ctypes.data, self._err, len(self._err)))

    def resolve(self, frames: int):
        """Final resolve of the owned rows into host arrays."""
        rows, w = self.rows, self.width
        rgba = np.zeros((rows, w, 4), np.uint8)
        alb = np.zeros((rows, w, 3), np.float32)
        nrm = np.zeros((rows, w, 3), np.float32)
        dep = np.zeros((rows, w), np.float32)
        valid = C.c_int32(0)
        self._check(self._lib.f3d_session_resolve(self._handle, int(frames), rgba.ctypes.data, alb.ctypes.data,
                                                  nrm.ctypes.data, dep.ctypes.data, C.byref(valid), self._err,
                                                  len(self._err)))
        return {"rgba": rgba, "albedo": alb, "normal": nrm, "depth": dep, "any_valid_reservoir": bool(valid.value)}

    def resolve_device(self, frames: int, d_rgba=0, d_albedo=0, d_normal=0, d_depth=0):
        self._check(self._lib.f3d_session_resolve_device(self._handle, int(frames), C.c_void_p(d_rgba or None),
                                                         C.c_void_p(d_albedo or None), C.c_void_p(d_normal or None),
                                                         C.c_void_p(d_depth or None), self._err, len(self._err)))

    def info(self):
        g, p, h = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rows, width = C.c_uint32(0), C.c_uint32(0)
        self._lib.f3d_session_info(self._handle, C.byref(g), C.byref(p), C.byref(h), C.byref(rows), C.byref(width))
        return {"gpu_resource_bytes": int(g.value), "minmax_pyramid_bytes": int(p.value),
                "peak_host_visible_bytes": int(h.value), "rows": int(rows.value), "width": int(width.value)}

    def setup_ms(self) -> dict:
        """Host wall time of the session's creation by phase (ms): what a render pays once before its first frame."""
        out = (C.c_double * 8)()
        self._lib.f3d_session_setup_ms(self._handle, out, 8)
        keys = ("total", "validate", "hash", "upload", "tables", "scene", "alloc", "passes")
        return {k: float(out[i]) for i, k in enumerate(keys)}

    def sample_lanes(self) -> int:
        """Sample lanes per pixel of the frame kernel (1, 2, 4 or 8; chosen from the strip size and spp)."""
        return int(self._lib.f3d_session_sample_lanes(self._handle))

    def row_costs(self) -> np.ndarray:
        """Cost of the last fused frame by image row of this strip (float32[rows], wave time in 100 MHz ticks); synchronises."""
        out = np.zeros(self.rows, np.float32)
        self._check(self._lib.f3d_session_row_costs(self._handle, out.ctypes.data_as(C.POINTER(C.c_float)), self.rows, self._err, len(self._err)))
        return out

    def primary_start_ptr(self) -> int:
        """Device pointer to the session's primary-ray certificates (rows x width records, f3d_cone.h), 0 if it has none; valid
        while the session lives.  The PBR path tracer takes it (WavefrontScene / f3d_wf_scene.primary_start)."""
        return int(self._lib.f3d_session_primary_start(self._handle) or 0)

    def kernel_timing(self, enable: bool):
        """enable=True starts recording a hipEvent pair around every frame launch;
        enable=False stops and returns (average ms per launch, launches)."""
        avg, n = C.c_double(0.0), C.c_uint32(0)
        rc = self._lib.f3d_session_kernel_timing(self._handle, 1 if enable else 0, C.byref(avg), C.byref(n))
        if rc != 0:
            raise RuntimeError("kernel timing failed")
        return float(avg.value), int(n.value)


def srgb_to_linear(image) -> np.ndarray:
    """The sRGB transfer function's inverse on the first three channels of a float32 image in [0, 1], in float32."""
    out = np.array(image, dtype=np.float32, copy=True)
    c = out[..., :3]
    low = c <= np.float32(0.04045)
    with np.errstate(invalid="ignore"):
        high = np.power((c + np.float32(0.055)) / np.float32(1.055), np.float32(2.4), dtype=np.float32)
    out[..., :3] = np.where(low, c / np.float32(12.92), high)
    return out


def kernel_variant(*, sample_lanes: int = 0, waves_per_simd: int = 0, tile_map: int = 0, leaf_quorum: int = 0, share_below: int = 0) -> int:
    """f3d_session_opts.kernel_variant from names (include/f3d_terrain_pt.h lists the decimal fields): every A/B switch of the
    frame kernel that is not a build flag.  All zero = the shipped default."""
    if sample_lanes not in (0, 1, 2, 4, 8):
        raise ValueError("sample_lanes must be 0 (automatic), 1, 2, 4 or 8")
    if waves_per_simd not in (0, 4, 5, 6):
        raise ValueError("waves_per_simd must be 0 / 6 (default), 4 (1 sample lane) or 5 (4 sample lanes)")
    if not (0 <= tile_map <= 4 and 0 <= leaf_quorum <= 64 and 0 <= share_below <= 64):
        raise ValueError("tile_map in 0..4, leaf_quorum and share_below in 0..64")
    budget = 0 if waves_per_simd in (0, 6) else 100 + waves_per_simd
    return budget + 1000 * tile_map + 10000 * leaf_quorum + 1000000 * sample_lanes + 10000000 * share_below


def describe_kernel_variant(v: int) -> dict:
    """The fields of a kernel_variant, by name."""
    v = int(v)
    budget = v % 1000
    return {"waves_per_simd": 6 if budget == 0 else (budget - 100), "tile_map": (v // 1000) % 10, "leaf_quorum": (v // 10000) % 100,
            "sample_lanes": (v // 1000000) % 10, "share_below": (v // 10000000) % 100}


def reservoir_buffer_bytes(rows: int, width: int) -> int:
    return (rows + 2 * HALO_ROWS) * width * RESERVOIR_BYTES
