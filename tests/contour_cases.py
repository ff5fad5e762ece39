"""What the contour tests share (tests/test_session_contour_host.py, tests/test_gpu_contour.py) -- TEST INFRASTRUCTURE ONLY:
the DEMs, regions and level lists at which the contour kernels can go wrong, and the kernels' lane bodies compiled for the
host (tests/contour_host), whose bits the device must return."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import scenes
from emul import emul
from test_session_raster_host import _kw, shaped_dem
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "contour_host" / "contour_harness.cpp"
SIZE = (64, 48)  # every render of the contour tests
f32 = np.float32

# (rows, cols) of the DEM and its spacing (None: the scenes' own): one cell; no level 3 in the pyramid; exactly one block;
# partial blocks; an anisotropic lattice; test_session_raster_host.SHAPES' 64x64 and 65x63
SHAPES = [((2, 2), None), ((3, 5), None), ((9, 9), None), ((9, 10), None), ((33, 33), (10.0, 7.0)), ((64, 64), None), ((63, 65), None)]
EXAGGERATIONS = (1.0, 2.5)


def shape_kw(dem, spacing=None, exaggeration=None):
    kw = _kw(dem)
    if spacing is not None:
        kw["spacing"] = tuple(spacing)
    if exaggeration is not None:
        kw["exaggeration"] = float(exaggeration)
    return kw


def regions(shape):
    """Cell regions of a DEM of `shape`: whole, one cell, strictly inside a block, crossing block borders unaligned."""
    cell_h, cell_w = shape[0] - 1, shape[1] - 1
    out = {"whole": (0, 0, cell_h, cell_w), "one cell": (cell_h - 1, cell_w - 1, 1, 1)}
    if cell_h >= 7 and cell_w >= 7:
        out["inside a block"] = (2, 1, 4, 5)
    if cell_h >= 20 and cell_w >= 20:
        out["across blocks"] = (5, 3, 13, 15)
    return out


def level_lists(h32, steep=True):
    """Level lists over session heights h32 (float32): each finite and strictly ascending."""
    lo, hi = float(h32.min()), float(h32.max())
    span = max(hi - lo, 1e-3)
    sample = float(h32[h32.shape[0] // 2, h32.shape[1] // 2])
    out = {
        "one": np.array([lo + 0.37 * span], f32),
        "interval": np.unique((lo + span * np.arange(1, 12) / 12.0).astype(f32)),
        "below": np.array([lo - 2.0 * span - 1.0, lo - span - 1.0], f32),
        "above": np.array([hi + span + 1.0, hi + 2.0 * span + 1.0], f32),
        "at the minimum": np.array([lo], f32),
        "at the maximum": np.array([hi], f32),
        "at a sample": np.unique(np.array([sample, sample + 0.25 * span], f32)),
    }
    if steep:  # the maximum count: every cell whose corners differ by more than span / 1000 crosses more than 64 levels
        out["maximum count"] = np.unique(np.linspace(lo - 0.01 * span, hi + 0.01 * span, 65536).astype(f32))
    return out


def cone(shape, spacing, top=400.0):
    """h = top - r over a lattice centred on the world's origin, as a session places it (float32 samples)."""
    rows, cols = shape
    x = (np.arange(cols) - 0.5 * (cols - 1)) * spacing[0]
    z = (np.arange(rows) - 0.5 * (rows - 1)) * spacing[1]
    return (top - np.sqrt(x[None, :] ** 2 + z[:, None] ** 2)).astype(f32)


def build_harness():
    lib = emul.build_harness(HARNESS, "contour_host")
    lib.contour_scene_create.restype = C.c_void_p
    lib.contour_scene_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.contour_scene_destroy.argtypes = [C.c_void_p]
    lib.contour_heights.argtypes = [C.c_void_p, C.c_void_p]
    lib.contour_run.restype = C.c_uint64
    lib.contour_run.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64] + [C.c_void_p] * 6
    lib.contour_desc_size.restype = C.c_uint32
    lib.contour_desc_size.argtypes = [C.c_int]
    return lib


class HostContours:
    """A scene as the emulator sets it up, and contour calls over it as the device answers them."""

    def __init__(self, lib, dem, kw, cam=None):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        d, keep = _desc(self.dem, SIZE, cam or scenes.CAM, kw)
        info, dims = np.zeros(4, f32), np.zeros(3, np.uint32)
        self.handle = lib.contour_scene_create(C.addressof(d), info.ctypes.data, dims.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin, self.spacing = (f32(info[0]), f32(info[1])), (f32(info[2]), f32(info[3]))
        self.cell_w, self.cell_h, self.mip_count = (int(v) for v in dims)
        self.heights = np.zeros(self.dem.shape, f32)
        lib.contour_heights(self.handle, self.heights.ctypes.data)
        self.heights.setflags(write=False)

    def close(self):
        self.lib.contour_scene_destroy(self.handle)

    def run(self, levels, region=None, cull=True, capacity=None, details=False, rgba=None):
        """The records of one call, in order.  capacity None: all of them.  rgba: the paint form (``prims``: (N, 20) uint32)."""
        lv = np.ascontiguousarray(levels, f32)
        row0, col0, rows, cols = (0, 0, self.cell_h, self.cell_w) if region is None else region
        head = (self.handle, row0, col0, rows, cols, lv.ctypes.data, lv.size, 1 if cull else 0)
        total = int(self.lib.contour_run(*head, 0, None, None, None, None, None, None))
        n = total if capacity is None else min(total, int(capacity))
        seg, idx = np.full((n + 1, 4), 77.0, f32), np.full(n + 1, 77, np.uint32)
        cells, cases = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
        col = None if rgba is None else np.ascontiguousarray(rgba, f32)
        prims = None if rgba is None else np.zeros((n + 1, 20), np.uint32)
        again = int(self.lib.contour_run(*head, n, seg.ctypes.data, idx.ctypes.data, None if prims is None else prims.ctypes.data,
                                         None if col is None else col.ctypes.data, cells.ctypes.data if details else None,
                                         cases.ctypes.data if details else None))
        assert again == total
        assert (seg[n] == 77.0).all() and idx[n] == 77, "nothing is written behind the capacity"
        out = {"segments": seg[:n], "level_index": idx[:n], "total": total}
        if details:
            out.update(cell=cells[:n].astype(np.int64), case=cases[:n].astype(np.int64))
        if prims is not None:
            out["prims"] = prims[:n]
        return out
