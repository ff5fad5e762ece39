"""What the drainage tests share (tests/test_session_drainage_host.py, tests/test_gpu_drainage.py) -- TEST INFRASTRUCTURE ONLY:
the DEMs and regions at which the drainage kernels can go wrong, and the kernels' lane bodies compiled for the host
(tests/drainage_host), whose bits the device must return."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import scenes
from contour_cases import EXAGGERATIONS, SHAPES, SIZE, cone, shape_kw  # noqa: F401  (the contour tests' shapes: 2x2 ... 63x65)
from emul import emul
from test_session_raster_host import shaped_dem  # noqa: F401
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "drainage_host" / "drainage_harness.cpp"
f32 = np.float32


def regions(shape):
    """Sample regions of a DEM of `shape`: whole, one sample, strictly inside a tile, crossing tile borders unaligned."""
    rows, cols = shape
    out = {"whole": (0, 0, rows, cols), "one sample": (rows - 1, cols - 1, 1, 1)}
    if rows >= 8 and cols >= 8:
        out["inside a tile"] = (2, 1, 4, 5)
    if rows >= 21 and cols >= 21:
        out["across tiles"] = (5, 3, 13, 15)
    return out


def ramp(shape=(9, 17)):
    """h = -2 i: every sample drains east, the last column holds the outlets."""
    return np.tile(np.arange(shape[1], dtype=f32) * f32(-2.0), (shape[0], 1))


def bowl(shape=(9, 9)):
    """h = r^2 around the middle sample: one sink that accumulates everything."""
    j, i = np.meshgrid(np.arange(shape[0]) - shape[0] // 2, np.arange(shape[1]) - shape[1] // 2, indexing="ij")
    return (i * i + j * j).astype(f32)


def flat(shape=(9, 10)):
    return np.full(shape, 3.0, f32)


def plateau_with_a_tie():
    """A 5 x 5 plateau at 10 whose middle sample stands at 11: its eight slopes tie in pairs (E = W, S = N; the diagonals are
    lower at any spacing), and with spacing_x = spacing_z all four cardinals tie: code 0, E, the lowest, wins."""
    dem = np.full((5, 5), 10.0, f32)
    dem[2, 2] = 11.0
    return dem


def serpentine(n=33, wall=1000.0, step=0.25):
    """Walls at `wall`; a channel along every second row (0, 2, ..., n - 1), eastward and westward in turn, joined at the rows'
    ends through one sample of the row between, descending `step` a sample to 0 at its end.  One sink, the channel's end;
    every wall sample drains into the channel row below it (the lower of its two).  Water cuts each corner diagonally -- the
    drop of two steps over a diagonal beats one step over a side --, so the longest path has 544 steps on 33 x 33."""
    dem = np.full((n, n), wall, f32)
    path = []
    for k, j in enumerate(range(0, n, 2)):
        cols = range(n) if k % 2 == 0 else range(n - 1, -1, -1)
        path += [(j, i) for i in cols]
        if j + 2 < n:
            path.append((j + 1, path[-1][1]))
    for idx, (j, i) in enumerate(path):
        dem[j, i] = step * (len(path) - 1 - idx)
    return dem


def build_harness():
    lib = emul.build_harness(HARNESS, "drainage_host")
    lib.drain_scene_create.restype = C.c_void_p
    lib.drain_scene_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.drain_scene_destroy.argtypes = [C.c_void_p]
    lib.drain_heights.argtypes = [C.c_void_p, C.c_void_p]
    lib.drain_run.restype = None
    lib.drain_run.argtypes = [C.c_void_p] * 6
    lib.stream_run.restype = C.c_uint64
    lib.stream_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 4
    lib.drain_desc_size.restype = C.c_uint32
    lib.drain_desc_size.argtypes = [C.c_int]
    return lib


class HostDrainage:
    """A scene as the emulator sets it up, and drainage calls over it as the device answers them."""

    def __init__(self, lib, dem, kw, cam=None):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        d, keep = _desc(self.dem, SIZE, cam or scenes.CAM, kw)
        info, dims = np.zeros(4, f32), np.zeros(3, np.uint32)
        self.handle = lib.drain_scene_create(C.addressof(d), info.ctypes.data, dims.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin, self.spacing = (f32(info[0]), f32(info[1])), (f32(info[2]), f32(info[3]))
        self.cell_w, self.cell_h, self.mip_count = (int(v) for v in dims)
        self.heights = np.zeros(self.dem.shape, f32)
        lib.drain_heights(self.handle, self.heights.ctypes.data)
        self.heights.setflags(write=False)

    def close(self):
        self.lib.drain_scene_destroy(self.handle)

    def _region(self, region):
        return np.array((0, 0) + self.dem.shape if region is None else region, np.uint32)

    def run(self, region=None):
        """{"direction", "accumulation", "basin" (rows, cols), "sinks", "rounds", "longest"} of one call."""
        reg = self._region(region)
        rows, cols = int(reg[2]), int(reg[3])
        d, a, b = np.full((rows, cols), 0xEE, np.uint8), np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
        stats = np.zeros(3, np.uint32)
        self.lib.drain_run(self.handle, reg.ctypes.data, d.ctypes.data, a.ctypes.data, b.ctypes.data, stats.ctypes.data)
        return {"direction": d, "accumulation": a, "basin": b, "sinks": int(stats[0]), "rounds": int(stats[1]), "longest": int(stats[2])}

    def streams(self, threshold, region=None, capacity=None, rgba=None):
        """The records of one stream call, in order.  capacity None: all.  rgba: the paint form (``prims``: (N, 20) uint32)."""
        reg = self._region(region)
        total = int(self.lib.stream_run(self.handle, reg.ctypes.data, threshold, 0, None, None, None, None))
        n = total if capacity is None else min(total, int(capacity))
        seg, acc = np.full((n + 1, 4), 77.0, f32), np.full(n + 1, 77, np.uint32)
        col = None if rgba is None else np.ascontiguousarray(rgba, f32)
        prims = None if rgba is None else np.zeros((n + 1, 20), np.uint32)
        again = int(self.lib.stream_run(self.handle, reg.ctypes.data, threshold, n, seg.ctypes.data, acc.ctypes.data,
                                        None if prims is None else prims.ctypes.data, None if col is None else col.ctypes.data))
        assert again == total
        assert (seg[n] == 77.0).all() and acc[n] == 77, "nothing is written behind the capacity"
        out = {"segments": seg[:n], "accumulation": acc[:n], "total": total}
        if prims is not None:
            out["prims"] = prims[:n]
        return out


def named_cases():
    """name -> (dem, spacing or None, exaggeration): the shaped proxies at both exaggerations, then the known answers."""
    out = {}
    for shape, spacing in SHAPES:
        for e in EXAGGERATIONS:
            out[f"{shape[1]}x{shape[0]} x{e}"] = (shaped_dem(shape), spacing, e)
    out["ramp"] = (ramp(), (5.0, 3.0), 1.0)
    out["bowl"] = (bowl(), None, 1.0)
    out["cone 63x65"] = (cone((63, 65), (10.0, 10.0)), (10.0, 10.0), 1.0)
    out["cone 33x33"] = (cone((33, 33), (10.0, 7.0)), (10.0, 7.0), 1.0)
    out["flat"] = (flat(), None, 1.0)
    out["plateau"] = (plateau_with_a_tie(), (10.0, 10.0), 1.0)
    out["serpentine"] = (serpentine(), (10.0, 10.0), 1.0)
    return out
