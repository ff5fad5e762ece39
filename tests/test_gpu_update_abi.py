"""`-m gpu`: a descriptor of another header revision at every door of a live session's updates.

f3d_session_rearm / _reaim / _remesh / _reterrain read a descriptor that nests the one before it (re-mesh and re-terrain
hold a re-aim descriptor, which holds a re-arm descriptor), and every level carries its own ``struct_size``.  A wrong size
at any level of any door is refused with status 1 and the text that names exactly that struct, before a member is read
and before the session changes: its fingerprint stays, and it then renders what a session that saw none of them renders.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scenes
from test_gpu_reaim import _same

pytestmark = pytest.mark.gpu

W, H = 32, 24
QUAD = (np.array([(-10.0, 30.0, -10.0), (10.0, 30.0, -10.0), (10.0, 30.0, 10.0), (-10.0, 30.0, 10.0)], np.float32),
        np.array([(0, 1, 2), (0, 2, 3)], np.uint32))
# door -> (path to a nested descriptor, the struct it is), outermost first
DOORS = {"rearm": [((), "f3d_session_rearm_desc")],
         "reaim": [((), "f3d_session_reaim_desc"), (("arm",), "f3d_session_rearm_desc")],
         "remesh": [((), "f3d_session_remesh_desc"), (("aim",), "f3d_session_reaim_desc"), (("aim", "arm"), "f3d_session_rearm_desc")],
         "reterrain": [((), "f3d_session_reterrain_desc"), (("aim",), "f3d_session_reaim_desc")]}


def _session():
    from forge3d_amd.session import TerrainSession

    dem = scenes.golden_dem(8)
    kw = scenes.fixed_frames(scenes.scene_kwargs(dem), 2, spp=1)
    return dem, TerrainSession(dem, W, H, dict(scenes.CAM), mesh_vertices=QUAD[0], mesh_indices=QUAD[1], **kw)


def _descriptor(s, door, dem):
    """A descriptor the door accepts as it stands (the session's own camera and values), and what its pointers name."""
    from forge3d_amd import _native

    aim = s._reaim_desc(s._camera, {})
    if door == "rearm":
        return aim.arm, None
    if door == "reaim":
        return aim, None
    d = {"remesh": _native.RemeshDesc, "reterrain": _native.ReterrainDesc}[door]()
    d.struct_size = C.sizeof(d)
    d.aim = aim
    if door == "remesh":
        d.mesh_vertices, d.mesh_vertex_count = QUAD[0].ctypes.data, len(QUAD[0])
        return d, QUAD
    d.heights, d.width, d.height = dem.ctypes.data, dem.shape[1], dem.shape[0]
    return d, dem


def test_struct_size_refusal_at_every_door():
    from forge3d_amd import _native

    lib = _native.lib()
    dem, s = _session()
    _, fresh = _session()
    with s, fresh:
        before = s.fingerprint()
        err = C.create_string_buffer(1024)
        refused = 0
        for door, levels in DOORS.items():
            for path, name in levels:
                d, keep = _descriptor(s, door, dem)
                level = d
                for member in path:
                    level = getattr(level, member)
                right = C.sizeof(level)
                level.struct_size = right + 8
                rc = getattr(lib, "f3d_session_" + door)(s._handle, C.byref(d), err, len(err))
                message = err.value.decode()
                assert rc == 1, f"{door} {path}: status {rc}, {message!r}"
                assert message == (f"{name}.struct_size is {right + 8}, this library (ABI version {_native.ABI_VERSION}) expects {right}: "
                                   "the caller was built against another revision of f3d_terrain_pt.h"), f"{door} {path}"
                with pytest.raises(ValueError, match=rf"^{name}\.struct_size is "):
                    _native.raise_status(rc, message)
                refused += 1
                del keep
        assert refused == 8
        assert s.fingerprint() == before
        _same(s.render(), fresh.render(), "after the refused descriptors")
