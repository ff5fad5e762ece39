"""ctypes binding of libf3dhip.so -- the C ABI declared in include/f3d_terrain_pt.h.

This module plays the role of the reference's compiled extension ``forge3d._forge3d``
for the one hot path it replaces: ``hybrid_render_terrain_reference`` below has the
native function's positional signature and defaults (reference
src/py_functions/path_tracing/terrain_reference.rs:224-256).  There is no CPU fallback:
when the shared library is missing or no HIP device is present the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libf3dhip.so"

STATUS_OK, STATUS_VALUE, STATUS_RENDER, STATUS_UPLOAD, STATUS_DEVICE = 0, 1, 2, 3, 4
ABI_VERSION = 6  # F3D_ABI_VERSION of include/f3d_terrain_pt.h this mirror was written against
FRAMES_IN_FLIGHT_AUTO = 0xFFFFFFFF  # f3d_session_opts.frames_in_flight: what f3d_terrain_ref_render uses

_EARTH = {"flat": 0, "sphere": 1, "ellipsoid": 2, "wgs84": 2}
_REFRACTION = {"none": 0, "bennett": 1, "saemundsson": 2, "effective_radius": 3}


class Desc(C.Structure):
    """f3d_terrain_ref_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("heights", C.c_void_p), ("dem_width", C.c_uint32), ("dem_height", C.c_uint32),
        ("spacing_x", C.c_float), ("spacing_z", C.c_float), ("exaggeration", C.c_float),
        ("albedo", C.c_float * 3),
        ("cam_origin", C.c_float * 3), ("cam_look_at", C.c_float * 3), ("cam_up", C.c_float * 3),
        ("fov_y_deg", C.c_float), ("exposure", C.c_float),
        ("sun_azimuth_deg", C.c_float), ("sun_elevation_deg", C.c_float), ("sun_intensity", C.c_float),
        ("sun_color", C.c_float * 3),
        ("observer_latitude_deg", C.c_double), ("observer_longitude_deg", C.c_double),
        ("earth_model", C.c_int32), ("refraction_model", C.c_int32),
        ("sphere_radius_m", C.c_double), ("refraction_k", C.c_double),
        ("pressure_mbar", C.c_double), ("temperature_c", C.c_double),
        ("env_map", C.c_void_p), ("env_width", C.c_uint32), ("env_height", C.c_uint32),
        ("env_intensity", C.c_float),
        ("mesh_vertices", C.c_void_p), ("mesh_vertex_count", C.c_uint32),
        ("mesh_indices", C.c_void_p), ("mesh_index_count", C.c_uint32),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("seed", C.c_uint32), ("spp", C.c_uint32), ("max_frames", C.c_uint32), ("min_frames", C.c_uint32),
        ("variance_threshold", C.c_float),
        ("atmosphere", C.c_void_p),
    ]


class AetherLuts(C.Structure):
    """f3d_aether_luts"""
    _fields_ = [
        ("transmittance", C.c_void_p), ("accumulated_scattering", C.c_void_p), ("aerial", C.c_void_p),
        ("transmittance_mu", C.c_uint32), ("transmittance_height", C.c_uint32),
        ("scattering_mu_view", C.c_uint32), ("scattering_mu_sun", C.c_uint32), ("scattering_height", C.c_uint32),
        ("scattering_nu", C.c_uint32),
        ("aerial_distance", C.c_uint32), ("aerial_mu_view", C.c_uint32), ("aerial_height", C.c_uint32),
        ("turbidity", C.c_float), ("ozone_du", C.c_float), ("mie_g", C.c_float), ("bottom_radius_m", C.c_float),
        ("top_radius_m", C.c_float), ("rayleigh_scale_height_m", C.c_float), ("mie_scale_height_m", C.c_float),
        ("max_aerial_distance_m", C.c_float), ("ground_albedo", C.c_float), ("scattering_orders", C.c_uint32),
    ]


class Out(C.Structure):
    """f3d_terrain_ref_out"""
    _fields_ = [
        ("rgba", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p),
        ("frames", C.c_uint32), ("variance", C.c_float), ("converged", C.c_int32),
        ("peak_host_visible_bytes", C.c_uint64), ("minmax_pyramid_bytes", C.c_uint64),
        ("gpu_resource_bytes", C.c_uint64),
        ("loop_seconds", C.c_double), ("setup_seconds", C.c_double), ("readback_seconds", C.c_double),
    ]


class HaloExport(C.Structure):
    """f3d_halo_export"""
    _fields_ = [("handle", (C.c_uint8 * 64) * 3), ("offset", C.c_uint64 * 3), ("address", C.c_uint64 * 3),
                ("rows", C.c_uint32), ("width", C.c_uint32), ("device", C.c_int32), ("pid", C.c_uint32)]


class HaloStats(C.Structure):
    """f3d_halo_stats"""
    _fields_ = [("reset", C.c_uint32), ("frames_published", C.c_uint32), ("timeouts", C.c_uint32), ("pulls", C.c_uint32),
                ("wait_ms", C.c_double * 2), ("longest_wait_ms", C.c_double), ("timeout_ms", C.c_double)]


class SessionOpts(C.Structure):
    """f3d_session_opts"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32), ("stream", C.c_void_p),
        ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
        ("memory_budget_bytes", C.c_uint64), ("kernel_variant", C.c_int32),
        ("ext_reservoirs", C.c_void_p * 2), ("ext_stats", C.c_void_p),
        ("bands", C.c_uint32), ("band_streams", C.c_uint32), ("mesh_builder", C.c_uint32), ("frames_in_flight", C.c_uint32),
    ]


class RearmDesc(C.Structure):
    """f3d_session_rearm_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("sun_azimuth_deg", C.c_float), ("sun_elevation_deg", C.c_float), ("sun_intensity", C.c_float),
        ("sun_color", C.c_float * 3),
        ("exposure", C.c_float), ("env_intensity", C.c_float),
        ("seed", C.c_uint32), ("max_frames", C.c_uint32), ("min_frames", C.c_uint32),
        ("variance_threshold", C.c_float),
        ("observer_latitude_deg", C.c_double), ("observer_longitude_deg", C.c_double),
        ("pressure_mbar", C.c_double), ("temperature_c", C.c_double),
    ]


class ReaimDesc(C.Structure):
    """f3d_session_reaim_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("cam_origin", C.c_float * 3), ("cam_look_at", C.c_float * 3), ("cam_up", C.c_float * 3),
        ("fov_y_deg", C.c_float),
        ("arm", RearmDesc),
    ]


class RemeshDesc(C.Structure):
    """f3d_session_remesh_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mesh_vertices", C.c_void_p), ("mesh_vertex_count", C.c_uint32),
        ("mesh_indices", C.c_void_p), ("mesh_index_count", C.c_uint32),
        ("aim", ReaimDesc),
    ]


class ReterrainDesc(C.Structure):
    """f3d_session_reterrain_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("heights", C.c_void_p),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("x0", C.c_uint32), ("y0", C.c_uint32),
        ("exaggeration", C.c_float),
        ("aim", ReaimDesc),
    ]


class QueryDesc(C.Structure):
    """f3d_session_query_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32), ("count", C.c_uint32),
        ("rays", C.c_void_p),
        ("kind", C.c_void_p), ("t", C.c_void_p), ("normal", C.c_void_p), ("position", C.c_void_p),
        ("primitive", C.c_void_p), ("direction", C.c_void_p),
    ]


QUERY_CLOSEST, QUERY_OCCLUSION, QUERY_PIXELS = 0, 1, 2
QUERY_TERRAIN_ONLY, QUERY_CURVED, QUERY_DEVICE_POINTERS, QUERY_NO_WAIT = 1, 2, 4, 8
QUERY_SCRATCH_BYTES_PER_RAY = 80  # F3D_QUERY_SCRATCH_BYTES_PER_RAY


class RasterDesc(C.Structure):
    """f3d_session_raster_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("lift", C.c_float), ("target_count", C.c_uint32), ("reserved", C.c_uint32),
        ("targets", C.c_void_p), ("masks", C.c_void_p), ("count", C.c_void_p),
    ]


RASTER_TOWARD_POINT, RASTER_ALONG_DIRECTION = 0, 1
RASTER_TERRAIN_ONLY, RASTER_CURVED, RASTER_DEVICE_POINTERS, RASTER_NO_WAIT, RASTER_SESSION_SUN = 1, 2, 4, 8, 16


class HorizonDesc(C.Structure):
    """f3d_session_horizon_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("lift", C.c_float), ("azimuth_count", C.c_uint32),
        ("azimuths", C.c_void_p), ("horizon", C.c_void_p), ("sky_view", C.c_void_p),
        ("reserved", C.c_uint32),
    ]


HORIZON_CURVED, HORIZON_DEVICE_POINTERS, HORIZON_NO_WAIT = 2, 4, 8
HORIZON_MAX_AZIMUTHS = 256  # F3D_HORIZON_MAX_AZIMUTHS


class IrradiationDesc(C.Structure):
    """f3d_session_irradiation_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("lift", C.c_float), ("direction_count", C.c_uint32),
        ("directions", C.c_void_p), ("energy", C.c_void_p), ("count", C.c_void_p), ("normal", C.c_void_p),
        ("reserved", C.c_uint32),
    ]


IRRADIATION_TERRAIN_ONLY, IRRADIATION_CURVED, IRRADIATION_DEVICE_POINTERS, IRRADIATION_NO_WAIT, IRRADIATION_HORIZONTAL = 1, 2, 4, 8, 16


class ClearanceDesc(C.Structure):
    """f3d_session_clearance_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("observer_count", C.c_uint32),
        ("observers", C.c_void_p), ("height", C.c_void_p), ("lowest", C.c_void_p),
        ("reserved", C.c_uint32),
    ]


CLEARANCE_CURVED, CLEARANCE_DEVICE_POINTERS, CLEARANCE_NO_WAIT = 2, 4, 8


class UmbraDesc(C.Structure):
    """f3d_session_umbra_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("direction_count", C.c_uint32), ("reserved", C.c_uint32),
        ("directions", C.c_void_p), ("depth", C.c_void_p), ("deepest", C.c_void_p),
    ]


UMBRA_CURVED, UMBRA_DEVICE_POINTERS, UMBRA_NO_WAIT, UMBRA_SESSION_SUN = 2, 4, 8, 16


class DrapeDesc(C.Structure):
    """f3d_session_drape_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("image", C.c_void_p),
        ("rows", C.c_uint32), ("cols", C.c_uint32), ("channels", C.c_uint32), ("filter", C.c_uint32),
        ("scale_x", C.c_float), ("offset_x", C.c_float), ("scale_z", C.c_float), ("offset_z", C.c_float),
        ("at_row", C.c_uint32), ("at_col", C.c_uint32),
        ("aim", ReaimDesc),
    ]


DRAPE_NEAREST, DRAPE_BILINEAR = 0, 1
DRAPE_DEVICE_POINTERS, DRAPE_NO_WAIT, DRAPE_PATCH = 4, 8, 16
DRAPE_MAX_SIDE = 16384  # F3D_DRAPE_MAX_SIDE
DRAPE_TEXEL_MAX = 65504.0  # the largest finite binary16


class PaintDesc(C.Structure):
    """f3d_session_paint_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("primitive", C.c_uint32), ("vertex_count", C.c_uint32),
        ("xz", C.c_void_p), ("rgba", C.c_void_p), ("feature", C.c_void_p),
        ("indices", C.c_void_p), ("index_count", C.c_uint32),
        ("half_width", C.c_float), ("opacity", C.c_float),
        ("aim", ReaimDesc),
    ]


PAINT_POINTS, PAINT_LINES, PAINT_TRIANGLES = 0, 1, 2
PAINT_MAX_PRIMITIVES = 1 << 24  # F3D_PAINT_MAX_PRIMITIVES


class ContoursDesc(C.Structure):
    """f3d_session_contours_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("level_count", C.c_uint32), ("reserved", C.c_uint32),
        ("levels", C.c_void_p), ("segments", C.c_void_p), ("level_index", C.c_void_p),
        ("capacity", C.c_uint64), ("total", C.c_void_p),
    ]


class PaintContoursDesc(C.Structure):
    """f3d_session_paint_contours_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("level_count", C.c_uint32), ("reserved", C.c_uint32),
        ("levels", C.c_void_p), ("total", C.c_void_p),
        ("rgba", C.c_float * 4), ("half_width", C.c_float), ("opacity", C.c_float),
        ("aim", ReaimDesc),
    ]


CONTOUR_DEVICE_POINTERS = 4
CONTOUR_MAX_LEVELS = 65536  # F3D_CONTOUR_MAX_LEVELS


class DrainageDesc(C.Structure):
    """f3d_session_drainage_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("direction", C.c_void_p), ("accumulation", C.c_void_p), ("basin", C.c_void_p),
        ("stats", C.c_void_p), ("ms", C.c_void_p),
        ("reserved", C.c_uint32),
    ]


class StreamsDesc(C.Structure):
    """f3d_session_streams_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("threshold", C.c_uint32), ("reserved", C.c_uint32),
        ("segments", C.c_void_p), ("accumulation", C.c_void_p),
        ("capacity", C.c_uint64), ("total", C.c_void_p),
    ]


class PaintStreamsDesc(C.Structure):
    """f3d_session_paint_streams_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("threshold", C.c_uint32), ("reserved", C.c_uint32),
        ("total", C.c_void_p),
        ("rgba", C.c_float * 4), ("half_width", C.c_float), ("opacity", C.c_float),
        ("aim", ReaimDesc),
    ]


class FillDesc(C.Structure):
    """f3d_session_fill_desc"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("row0", C.c_uint32), ("col0", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
        ("filled", C.c_void_p), ("depth", C.c_void_p), ("flat_distance", C.c_void_p),
        ("stats", C.c_void_p), ("ms", C.c_void_p),
        ("reserved", C.c_uint32),
    ]


DRAINAGE_DEVICE_POINTERS = STREAMS_DEVICE_POINTERS = FILL_DEVICE_POINTERS = 4
DRAINAGE_FILL = STREAMS_FILL = 8  # F3D_DRAINAGE_FILL, F3D_STREAMS_FILL
DRAINAGE_SINK = 8  # F3D_DRAINAGE_SINK


# every symbol include/f3d_terrain_pt.h and include/f3d_wavefront.h declare: (name, restype, argtypes)
_P = C.POINTER
ABI = [
    ("f3d_terrain_ref_render", C.c_int, [_P(Desc), _P(Out), C.c_char_p, C.c_size_t]),
    ("f3d_session_create", C.c_int, [_P(Desc), _P(SessionOpts), _P(C.c_void_p), C.c_char_p, C.c_size_t]),
    ("f3d_session_destroy", None, [C.c_void_p]),
    ("f3d_session_enqueue_frames", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_char_p, C.c_size_t]),
    ("f3d_session_enqueue_trace", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    ("f3d_session_enqueue_merge", C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.c_char_p, C.c_size_t]),
    ("f3d_session_set_accumulation", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_session_halo_export", C.c_int, [C.c_void_p, _P(HaloExport), C.c_char_p, C.c_size_t]),
    ("f3d_session_halo_connect", C.c_int, [C.c_void_p, C.c_int32, _P(HaloExport), C.c_char_p, C.c_size_t]),
    ("f3d_session_halo_probe", C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, _P(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("f3d_session_halo_status", C.c_int, [C.c_void_p, _P(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("f3d_session_halo_stats", C.c_int, [C.c_void_p, _P(HaloStats), C.c_char_p, C.c_size_t]),
    ("f3d_session_enqueue_batch_strip", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_char_p, C.c_size_t]),
    ("f3d_session_frames_in_flight", C.c_uint32, [C.c_void_p]),
    ("f3d_session_retraced_pixels", C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    ("f3d_session_trace_batch", C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32]),
    ("f3d_session_window_stats", C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_int32), C.c_char_p, C.c_size_t]),
    ("f3d_scene_cache_limit", None, [C.c_uint32]),
    ("f3d_scene_cache_entries", C.c_uint32, []),
    ("f3d_wavefront_render", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                       C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_aether_bake", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_double),
                                  C.c_char_p, C.c_size_t]),
    ("f3d_smoke_render", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_smoke_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_aether_reference_render", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_smoke_composite", C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_session_fingerprint", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("f3d_session_mesh_tree", C.c_int, [C.c_void_p, _P(C.c_uint32), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    # re-arm of a live session (no ABI version bump: detected by the symbol)
    ("f3d_session_rearm", C.c_int, [C.c_void_p, _P(RearmDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_render", C.c_int, [C.c_void_p, _P(Out), C.c_char_p, C.c_size_t]),
    ("f3d_session_reaim", C.c_int, [C.c_void_p, _P(ReaimDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_remesh", C.c_int, [C.c_void_p, _P(RemeshDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_reterrain", C.c_int, [C.c_void_p, _P(ReterrainDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_query", C.c_int, [C.c_void_p, _P(QueryDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_raster", C.c_int, [C.c_void_p, _P(RasterDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_horizon", C.c_int, [C.c_void_p, _P(HorizonDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_irradiation", C.c_int, [C.c_void_p, _P(IrradiationDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_clearance", C.c_int, [C.c_void_p, _P(ClearanceDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_umbra", C.c_int, [C.c_void_p, _P(UmbraDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_drape", C.c_int, [C.c_void_p, _P(DrapeDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_draped", C.c_int, [C.c_void_p, _P(C.c_uint32)]),
    ("f3d_session_paint", C.c_int, [C.c_void_p, _P(PaintDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_paint_stats", C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_uint64)]),
    ("f3d_session_contours", C.c_int, [C.c_void_p, _P(ContoursDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_paint_contours", C.c_int, [C.c_void_p, _P(PaintContoursDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_drainage", C.c_int, [C.c_void_p, _P(DrainageDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_streams", C.c_int, [C.c_void_p, _P(StreamsDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_paint_streams", C.c_int, [C.c_void_p, _P(PaintStreamsDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_fill", C.c_int, [C.c_void_p, _P(FillDesc), C.c_char_p, C.c_size_t]),
    ("f3d_session_drape_read", C.c_int, [C.c_void_p, _P(C.c_uint32), C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_session_certificates", C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    ("f3d_session_sky_blocks", C.c_int, [C.c_void_p, _P(C.c_uint32)]),
    ("f3d_session_debug_wave_times", C.c_int, [C.c_void_p, C.c_void_p]),
    ("f3d_session_halo", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(C.c_void_p), _P(C.c_uint64)]),
    ("f3d_session_resolve", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      _P(C.c_int32), C.c_char_p, C.c_size_t]),
    ("f3d_session_resolve_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_session_setup_ms", C.c_int, [C.c_void_p, _P(C.c_double), C.c_uint32]),
    ("f3d_session_info", C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint32),
                                   _P(C.c_uint32)]),
    ("f3d_session_kernel_timing", C.c_int, [C.c_void_p, C.c_int32, _P(C.c_double), _P(C.c_uint32)]),
    ("f3d_session_sample_lanes", C.c_uint32, [C.c_void_p]),
    ("f3d_session_row_costs", C.c_int, [C.c_void_p, _P(C.c_float), C.c_uint32, C.c_char_p, C.c_size_t]),
    ("f3d_session_primary_start", C.c_void_p, [C.c_void_p]),
    ("f3d_smoke_set_stream", None, [C.c_void_p]),
    ("f3d_smoke_wait_fields_read", C.c_int, [C.c_void_p]),
    # a resident smoke sequence behind a handle (ABI 6)
    ("f3d_smoke_seq_create", C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_void_p), C.c_char_p, C.c_size_t]),
    ("f3d_smoke_seq_destroy", None, [C.c_void_p]),
    ("f3d_smoke_seq_streams", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    ("f3d_smoke_seq_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_smoke_seq_render", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_smoke_seq_composite", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_smoke_seq_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_halo_rows", C.c_uint32, []),
    ("f3d_session_enqueue_frame_part", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_char_p, C.c_size_t]),
    ("f3d_atrous_denoise", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_char_p, C.c_size_t]),
    ("f3d_build_minmax_mips", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                        _P(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("f3d_terrain_trace_batch", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p,
                                          C.c_size_t]),
    ("f3d_effective_radius_m", C.c_int, [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double,
                                         C.c_double, C.c_double, _P(C.c_double), C.c_char_p, C.c_size_t]),
    ("f3d_device_count", C.c_int, []),
    ("f3d_device_name", C.c_char_p, [C.c_int32]),
    ("f3d_version", C.c_char_p, []),
    ("f3d_abi_version", C.c_uint32, []),
    ("f3d_device_pool_trim", None, []),
    ("f3d_source_digest", C.c_char_p, []),
    ("f3d_debug_poison", None, [C.c_int32]),
]

_lib = None


def library_path() -> Path:
    return Path(os.environ.get("F3D_HIP_LIBRARY", str(LIB_PATH)))


HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    # numerics contract: no implicit FMA contraction on host or device
    "-ffp-contract=off",
    # the SLP vectoriser pairs independent f32 operations into v_pk_* instructions; on the 80-VGPR frame kernel
    # that costs register pairs and moves: 5763 -> 6362 Msamples/s without it (profiles/README.md)
    "-fno-slp-vectorize",
]
# only for f3d_kernels.hip (the frame kernels; compiled to an object first, then linked with the rest):
KERNEL_FLAGS = [
    # (round 3 switched the "VGPR live-range optimisation for if-else structures" off for this translation unit,
    # `-mllvm -amdgpu-opt-vgpr-liverange=false`: the frame kernel then spilled less inside the march's divergent regions, +1.5 %.
    # Round 4 took the spills out at the source -- 160 -> 12 bytes of scratch per lane -- and with them the reason: the
    # default is now 1.1 % FASTER, 8 690 -> 8 785 Msamples/s in one call, same image; profiles/r04_variant_ab.log)
]
HIP_SOURCES = ["f3d_kernels.hip", "f3d_host.hip", "f3d_denoise.hip", "f3d_smoke.hip", "f3d_smoke_sim.hip", "f3d_composite.hip", "f3d_lbvh.hip", "f3d_bvh_refit.hip", "f3d_retable.hip", "f3d_wavefront.hip",
               "f3d_aether_bake.hip", "f3d_aether_ref.hip", "f3d_paint.hip", "f3d_contour.hip", "f3d_drainage.hip", "f3d_fill.hip"]


def source_digest() -> str:
    """What f3d_source_digest() of a library built NOW would return: SHA-256 over the compiler flags, every file of
    csrc/ and include/ (names and bytes), first 16 hex digits.  None when the sources are not next to the package."""
    import hashlib

    csrc, inc = _PKG / "csrc", _PKG.parent / "include"
    if not csrc.is_dir() or not inc.is_dir():
        return None
    h = hashlib.sha256(" ".join(HIPCC_FLAGS + KERNEL_FLAGS + HIP_SOURCES).encode())
    for f in sorted(csrc.glob("*.h")) + sorted(csrc.glob("*.hip")) + sorted(inc.glob("*.h")):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def _hipcc() -> str:
    import shutil

    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (expected /opt/rocm/bin/hipcc)")


def built_digest(path: Path = None):
    """f3d_source_digest() of an existing library, asked in a child process (loading needs no GPU); None if it cannot say."""
    import subprocess
    import sys

    path = Path(path or LIB_PATH)
    if not path.exists():
        return None
    probe = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.f3d_source_digest.restype = ctypes.c_char_p; "
             "print(L.f3d_source_digest().decode())")
    proc = subprocess.run([sys.executable, "-c", probe, str(path)], capture_output=True, text=True)
    return proc.stdout.strip() if proc.returncode == 0 else None


def build_library(force: bool = False) -> Path:
    """Compile libf3dhip.so for gfx950 next to the package (hipcc cross-compiles without a GPU) unless the one that is
    there was built from exactly these sources and flags."""
    import subprocess

    digest = source_digest()
    if digest is None:
        raise RuntimeError("forge3d_amd: the sources (forge3d_amd/csrc, include/) are not next to the package")
    if force or built_digest(LIB_PATH) != digest:
        csrc = _PKG / "csrc"
        tmp = LIB_PATH.with_name(f"{LIB_PATH.name}.{os.getpid()}.tmp")  # several ranks may find the library stale at once
        obj = LIB_PATH.with_name(f"f3d_kernels.{os.getpid()}.o")
        define = f'-DF3D_SOURCE_DIGEST="{digest}"'
        compile_only = [f for f in HIPCC_FLAGS if f != "-shared"]
        cmds = [[_hipcc(), *compile_only, *KERNEL_FLAGS, define, "-c", str(csrc / HIP_SOURCES[0]), "-o", str(obj)],
                # (the object first: hipcc puts a sticky `-x hip` in front of every .hip it is given)
                [_hipcc(), *HIPCC_FLAGS, define, str(obj), *(str(csrc / n) for n in HIP_SOURCES[1:]), "-o", str(tmp)]]
        try:
            for cmd in cmds:
                proc = subprocess.run(cmd, capture_output=True, text=True)
                if proc.returncode != 0:
                    tmp.unlink(missing_ok=True)
                    raise RuntimeError("hipcc failed:\n" + proc.stdout + proc.stderr)
        finally:
            obj.unlink(missing_ok=True)
        os.replace(tmp, LIB_PATH)
    return LIB_PATH


def lib() -> C.CDLL:
    """Load libf3dhip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        path = library_path()
        if not path.exists():
            raise RuntimeError(
                f"forge3d_amd: HIP library {path} is missing -- run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback"
            )
        # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64; if this
        # library pulled in /opt/rocm's copy first, a later `import torch` would find no GPUs.
        # Importing torch first makes both resolve to the same runtime (torch is plumbing for
        # device memory / streams / RCCL here, not part of the render path).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # what runs must be what is in the tree: a library next to its sources has to be built from exactly them (an
        # A/B library named by F3D_HIP_LIBRARY is the caller's own business).  A stale one is rebuilt here and now --
        # before it is loaded, a loaded library cannot be replaced -- and the rebuild says so on stderr.
        if "F3D_HIP_LIBRARY" not in os.environ:
            want = source_digest()
            if want is not None:
                have = built_digest(path)
                if have != want:
                    import sys

                    print(f"forge3d_amd: {path.name} was built from other sources (digest {have}, tree {want}): rebuilding",
                          file=sys.stderr, flush=True)
                    build_library(force=True)
        L = C.CDLL(str(path))
        for name, restype, argtypes in ABI:
            fn = getattr(L, name)  # AttributeError if the export is missing
            fn.restype = restype
            fn.argtypes = argtypes
        if L.f3d_abi_version() != ABI_VERSION:
            raise RuntimeError(f"forge3d_amd: {path} speaks ABI version {L.f3d_abi_version()}, this binding {ABI_VERSION}")
        want = source_digest() if "F3D_HIP_LIBRARY" not in os.environ else None
        have = L.f3d_source_digest().decode()
        if want is not None and have != want:
            raise RuntimeError(f"forge3d_amd: {path} was built from other sources (digest {have}, tree {want}) and could not be rebuilt")
        _lib = L
    return _lib


def debug_poison(pattern: int) -> None:
    """Diagnostics: fill every device buffer allocated from now on (and guard regions around it) with this byte;
    a negative pattern switches it off.  Results must not depend on it (csrc/f3d_devmem.h)."""
    lib().f3d_debug_poison(int(pattern))


def raise_status(status: int, message: str):
    """Map a C-ABI status to the exception the reference raises (src/core/error.rs:48-76)."""
    if status == STATUS_VALUE:
        raise ValueError(message)
    category = {STATUS_RENDER: "Render", STATUS_UPLOAD: "Upload", STATUS_DEVICE: "Device"}.get(status, "Render")
    raise RuntimeError(f"[{category}] {category} error: {message}")


def _f3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


def _extract_sun_color(obj):
    """extract_sun_color, terrain_reference.rs:12-43"""
    msg = "sun_color must be exactly three finite, non-negative numbers"
    if isinstance(obj, (str, bytes, bytearray, memoryview)):
        raise ValueError(msg)
    try:
        items = list(iter(obj))
    except TypeError:
        raise ValueError(msg)
    if len(items) != 3:
        raise ValueError(msg)
    out = []
    for item in items:
        if isinstance(item, (str, bytes, bytearray, memoryview)):
            raise ValueError(msg)
        try:
            v = float(item)
        except (TypeError, ValueError):
            raise ValueError(msg)
        out.append(float(np.float32(v)))
    if any((not np.isfinite(c)) or c < 0.0 for c in out):
        raise ValueError(msg)
    return out


def _resolve_atmosphere(atmosphere):
    """extract_atmosphere_lut_handle, terrain_reference.rs:45-219 -> forge3d_amd.atmosphere.resolve_setting"""
    if atmosphere is None:
        return None
    from .atmosphere import resolve_setting

    return resolve_setting(atmosphere)


def attach_atmosphere(desc, handle, keep):
    """Point desc.atmosphere at an f3d_aether_luts built from an AtmosphereLutHandle (keep-alives appended)."""
    if handle is None:
        return
    luts = AetherLuts()
    tables = [np.ascontiguousarray(t, dtype=np.uint16) for t in (handle.transmittance, handle.accumulated_scattering,
                                                                  handle.aerial_perspective)]
    luts.transmittance, luts.accumulated_scattering, luts.aerial = (t.ctypes.data for t in tables)
    dims, cfg = handle.config.dimensions, handle.config
    for name in ("transmittance_mu", "transmittance_height", "scattering_mu_view", "scattering_mu_sun", "scattering_height",
                 "scattering_nu", "aerial_distance", "aerial_mu_view", "aerial_height"):
        setattr(luts, name, int(getattr(dims, name)))
    for name in ("turbidity", "ozone_du", "mie_g", "bottom_radius_m", "top_radius_m", "rayleigh_scale_height_m",
                 "mie_scale_height_m", "max_aerial_distance_m", "ground_albedo"):
        setattr(luts, name, float(getattr(cfg, name)))
    luts.scattering_orders = int(cfg.scattering_orders)
    keep += tables + [luts]
    desc.atmosphere = C.addressof(luts)


def camera_members(cam):
    """The camera dict as a descriptor holds it -- (cam_origin, cam_look_at, cam_up, fov_y_deg, exposure) -- with the
    wrapper's defaults for missing keys: read by make_desc for a new session and by TerrainSession.reaim for a live one."""
    return (_f3(cam.get("origin", (0.0, 50.0, 120.0))), _f3(cam.get("look_at", (0.0, 0.0, 0.0))),
            _f3(cam.get("up", (0.0, 1.0, 0.0))), float(cam.get("fov_y", 45.0)), float(cam.get("exposure", 1.0)))


def make_desc(heightmap, width, height, cam, spacing, exaggeration, albedo, sun_azimuth_deg, sun_elevation_deg,
              sun_intensity, env_map, env_intensity, mesh_vertices, mesh_indices, spp, max_frames, min_frames,
              variance_threshold, seed, sun_color, observer_latitude_deg, observer_longitude_deg, earth_model,
              sphere_radius_m, refraction_model, refraction_k, pressure_mbar, temperature_c, atmosphere=None):
    """Build the C descriptor; returns (desc, keepalive list).  atmosphere: an AtmosphereLutHandle or None."""
    dem = np.ascontiguousarray(heightmap, dtype=np.float32)
    if dem.ndim != 2:
        raise TypeError("heightmap must be a 2-D float32 array")
    if earth_model not in _EARTH:
        raise ValueError(f"unsupported earth_model {earth_model!r}")
    if refraction_model not in _REFRACTION:
        raise ValueError(f"unsupported refraction_model {refraction_model!r}")
    keep = [dem]
    d = Desc()
    d.struct_size = C.sizeof(Desc)
    d.heights = dem.ctypes.data
    d.dem_height, d.dem_width = dem.shape
    d.spacing_x, d.spacing_z = float(spacing[0]), float(spacing[1])
    d.exaggeration = float(exaggeration)
    d.albedo = _f3(albedo)
    d.cam_origin, d.cam_look_at, d.cam_up, d.fov_y_deg, d.exposure = camera_members(cam)
    d.sun_azimuth_deg = float(sun_azimuth_deg)
    d.sun_elevation_deg = float(sun_elevation_deg)
    d.sun_intensity = float(sun_intensity)
    d.sun_color = _f3(sun_color)
    d.observer_latitude_deg = float(observer_latitude_deg)
    d.observer_longitude_deg = float(observer_longitude_deg)
    d.earth_model = _EARTH[earth_model]
    d.refraction_model = _REFRACTION[refraction_model]
    d.sphere_radius_m = float(sphere_radius_m)
    d.refraction_k = float(refraction_k)
    d.pressure_mbar = float(pressure_mbar)
    d.temperature_c = float(temperature_c)
    if env_map is not None:
        env = np.ascontiguousarray(env_map, dtype=np.float32)
        if env.ndim != 3 or env.shape[2] != 3:
            raise ValueError("env_map must have shape (H, W, 3)")
        keep.append(env)
        d.env_map = env.ctypes.data
        d.env_height, d.env_width = env.shape[0], env.shape[1]
    d.env_intensity = float(env_intensity)
    if (mesh_vertices is None) != (mesh_indices is None):
        raise ValueError("mesh_vertices and mesh_indices must be provided together")
    if mesh_vertices is not None:
        mv = np.ascontiguousarray(mesh_vertices, dtype=np.float32)
        mi = np.ascontiguousarray(mesh_indices, dtype=np.uint32)
        if mv.ndim != 2 or mv.shape[1] != 3:
            raise ValueError("mesh_vertices must have shape (N, 3)")
        if mi.ndim != 2 or mi.shape[1] != 3:
            raise ValueError("mesh_indices must have shape (M, 3)")
        keep += [mv, mi]
        d.mesh_vertices = mv.ctypes.data
        d.mesh_vertex_count = mv.shape[0]
        d.mesh_indices = mi.ctypes.data
        d.mesh_index_count = mi.size
    if int(width) < 0 or int(height) < 0 or int(spp) < 0 or int(max_frames) < 0 or int(min_frames) < 0 or int(seed) < 0:
        raise OverflowError("can't convert negative int to unsigned")
    d.width, d.height = int(width), int(height)
    d.seed, d.spp = int(seed), int(spp)
    d.max_frames, d.min_frames = int(max_frames), int(min_frames)
    d.variance_threshold = float(variance_threshold)
    attach_atmosphere(d, atmosphere, keep)
    return d, keep


def hybrid_render_terrain_reference(heightmap, width, height, cam, spacing=(1.0, 1.0), exaggeration=1.0,
                                    albedo=(0.6, 0.6, 0.6), sun_azimuth_deg=315.0, sun_elevation_deg=45.0,
                                    sun_intensity=2.5, env_map=None, env_intensity=0.35, mesh_vertices=None,
                                    mesh_indices=None, spp=1, max_frames=512, min_frames=32,
                                    variance_threshold=1e-3, seed=7, certificate=None, sun_color=None, cache=None,
                                    observer_latitude_deg=0.0, observer_longitude_deg=0.0, earth_model="ellipsoid",
                                    sphere_radius_m=6371008.8, refraction_model="bennett", refraction_k=0.13,
                                    pressure_mbar=1013.25, temperature_c=15.0, atmosphere=None):
    """Native seam: numpy in -> dict of numpy out (terrain_reference.rs:257-456), executed by
    hand-written HIP kernels on gfx950 through ``f3d_terrain_ref_render``."""
    _ = cache, certificate  # accepted and ignored (SURVEY.md 8b "side channels")
    sun = [1.0, 0.97, 0.92] if sun_color is None else _extract_sun_color(sun_color)
    aether = _resolve_atmosphere(atmosphere)
    d, keep = make_desc(heightmap, width, height, cam, spacing, exaggeration, albedo, sun_azimuth_deg,
                        sun_elevation_deg, sun_intensity, env_map, env_intensity, mesh_vertices, mesh_indices, spp,
                        max_frames, min_frames, variance_threshold, seed, sun, observer_latitude_deg,
                        observer_longitude_deg, earth_model, sphere_radius_m, refraction_model, refraction_k,
                        pressure_mbar, temperature_c, aether)
    L = lib()
    h, w = int(height), int(width)
    rgba = np.zeros((h, w, 4), np.uint8)
    alb = np.zeros((h, w, 3), np.float32)
    nrm = np.zeros((h, w, 3), np.float32)
    dep = np.zeros((h, w), np.float32)
    o = Out()
    o.rgba, o.albedo, o.normal, o.depth = rgba.ctypes.data, alb.ctypes.data, nrm.ctypes.data, dep.ctypes.data
    err = C.create_string_buffer(1024)
    rc = L.f3d_terrain_ref_render(C.byref(d), C.byref(o), err, len(err))
    del keep
    if rc != 0:
        raise_status(rc, err.value.decode("utf-8", "replace"))
    return result_dict(rgba, alb, nrm, dep, o, sun_azimuth_deg, sun_elevation_deg)


def result_dict(rgba, alb, nrm, dep, o, sun_azimuth_deg, sun_elevation_deg):
    """The result dict of a render (f3d_terrain_ref_render, f3d_session_render) from its arrays and f3d_terrain_ref_out."""
    return {
        "rgba": rgba, "albedo": alb, "normal": nrm, "depth": dep,
        "frames": int(o.frames), "variance": float(o.variance), "converged": bool(o.converged),
        "peak_host_visible_bytes": int(o.peak_host_visible_bytes),
        "minmax_pyramid_bytes": int(o.minmax_pyramid_bytes),
        "gpu_resource_bytes": int(o.gpu_resource_bytes),
        "sun_source": "manual_angles",
        "solar_azimuth_deg": float(sun_azimuth_deg), "solar_elevation_deg": float(sun_elevation_deg),
        # extra diagnostics (not in the reference dict): timings of the three phases
        "loop_seconds": float(o.loop_seconds), "setup_seconds": float(o.setup_seconds),
        "readback_seconds": float(o.readback_seconds),
    }


def global_memory_metrics():
    """Subset of `_forge3d.global_memory_metrics` the hot-path test reads
    (reference tests/test_hybrid_terrain_pt.py:387-408): the 512 MiB budget."""
    return {"limit_bytes": 512 << 20}


def device_count() -> int:
    return int(lib().f3d_device_count())
