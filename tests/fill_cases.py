"""What the fill tests share (tests/test_session_fill_host.py, tests/test_gpu_fill.py) -- TEST INFRASTRUCTURE ONLY: the DEMs at
which the filled routing can go wrong, and the fill kernels' lane and tile bodies compiled for the host (tests/fill_host),
whose bits the device must return."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import drainage_cases as cases
import scenes
from emul import emul
from test_session_rearm_host import _desc

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "fill_host" / "fill_harness.cpp"
f32 = np.float32
SMALL = 8  # the second tile edge the harness instantiates


def pit():
    """5 x 5, a plane that falls towards the last corner, h = 10 - i - j, with the middle sample dug to 3, below its lowest
    neighbour (4): one filled sample, and one sink, the corner, that collects all 25."""
    j, i = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    dem = (10 - i - j).astype(f32)
    dem[2, 2] = 3.0
    return dem


def nested():
    """9 x 9, the border at 0: a rim (8) with a notch (6) round a lake floor (5, one hole at 2) -- the outer lake, which
    spills through the notch at 6 --, and in its middle an island ring (7) round a pit (1): the inner lake, which spills over
    the ring into the outer one at 7.  Two spill levels."""
    dem = np.zeros((9, 9), f32)
    dem[1:8, 1:8] = 8.0
    dem[1, 4] = 6.0
    dem[2:7, 2:7] = 5.0
    dem[2, 2] = 2.0
    dem[3:6, 3:6] = 7.0
    dem[4, 4] = 1.0
    return dem


def relief(shape, seed):
    """Random relief with many depressions: smooth waves plus noise quantised to 0.5 (flats and ties)."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    h = 6.0 * np.sin(0.21 * i + 0.4) * np.cos(0.17 * j) + 0.05 * i + rng.normal(0.0, 1.5, shape)
    return (np.round(h * 2.0) / 2.0).astype(f32)


def walled_serpentine(n=33, frame=2000.0, step=0.25):
    """drainage_cases.serpentine's channel, ASCENDING `step` a sample from 0 at its start to its end, inside a frame one sample
    wide at `frame`; the frame has one gap, next to the channel's end (below it on the map) and 1 above it in height.  The
    whole channel is one lake at the gap's level, whose only way out is the gap: T grows along the channel from its end."""
    inner = cases.serpentine(n, step=step)
    channel = inner < 1000.0
    top = inner[channel].max()
    inner[channel] = top - inner[channel]
    dem = np.full((n + 2, n + 2), frame, f32)
    dem[1:-1, 1:-1] = inner
    end_j, end_i = np.unravel_index(np.argmax(np.where(channel, inner, -1.0)), inner.shape)
    assert end_j == n - 1
    dem[n + 1, end_i + 1] = top + 1.0
    return dem


def build_harness():
    lib = emul.build_harness(HARNESS, "fill_host")
    lib.fill_scene_create.restype = C.c_void_p
    lib.fill_scene_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fill_scene_destroy.argtypes = [C.c_void_p]
    lib.fill_heights.argtypes = [C.c_void_p, C.c_void_p]
    lib.fill_run.restype = None
    lib.fill_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    lib.fill_drain_run.restype = None
    lib.fill_drain_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    lib.fill_stream_run.restype = C.c_uint64
    lib.fill_stream_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 4
    lib.fill_desc_size.restype = C.c_uint32
    lib.fill_tile_edge.restype = C.c_uint32
    return lib


class HostFill:
    """A scene as the emulator sets it up, and fill / filled drainage calls over it as the device answers them.  ``edge``: the
    tile edge (None: the device's; 0 in drainage() and streams(): without the fill); ``seed``: the order of a round's tiles."""

    def __init__(self, lib, dem, kw, cam=None):
        self.lib = lib
        self.dem = np.ascontiguousarray(dem, f32)
        self.kw = kw
        self.tile = int(lib.fill_tile_edge())
        d, keep = _desc(self.dem, cases.SIZE, cam or scenes.CAM, kw)
        info, dims = np.zeros(4, f32), np.zeros(3, np.uint32)
        self.handle = lib.fill_scene_create(C.addressof(d), info.ctypes.data, dims.ctypes.data)
        del keep
        assert self.handle, "the scene's descriptor was refused"
        self.origin, self.spacing = (f32(info[0]), f32(info[1])), (f32(info[2]), f32(info[3]))
        self.heights = np.zeros(self.dem.shape, f32)
        lib.fill_heights(self.handle, self.heights.ctypes.data)
        self.heights.setflags(write=False)

    def close(self):
        self.lib.fill_scene_destroy(self.handle)

    def _region(self, region):
        return np.array((0, 0) + self.dem.shape if region is None else region, np.uint32)

    def _edge(self, edge):
        return self.tile if edge is None else int(edge)

    def fill(self, region=None, edge=None, seed=0):
        reg = self._region(region)
        shape = (int(reg[2]), int(reg[3]))
        W, D, T = np.full(shape, -7.0, f32), np.full(shape, -7.0, f32), np.full(shape, 0xEE, np.uint32)
        stats = np.zeros(4, np.uint32)
        self.lib.fill_run(self.handle, self._edge(edge), seed, reg.ctypes.data, W.ctypes.data, D.ctypes.data, T.ctypes.data, stats.ctypes.data)
        return {"filled": W, "depth": D, "flat_distance": T, "filled_samples": int(stats[0]), "fill_rounds": int(stats[1]), "flat_rounds": int(stats[2]),
                "largest_flat_distance": int(stats[3])}

    def drainage(self, region=None, edge=None, seed=0):
        reg = self._region(region)
        shape = (int(reg[2]), int(reg[3]))
        d, a, b = np.full(shape, 0xEE, np.uint8), np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        stats = np.zeros(3, np.uint32)
        self.lib.fill_drain_run(self.handle, self._edge(edge), seed, reg.ctypes.data, d.ctypes.data, a.ctypes.data, b.ctypes.data, stats.ctypes.data)
        return {"direction": d, "accumulation": a, "basin": b, "sinks": int(stats[0]), "rounds": int(stats[1]), "longest": int(stats[2])}

    def streams(self, threshold, region=None, edge=None, seed=0, rgba=None):
        reg = self._region(region)
        e = self._edge(edge)
        n = int(self.lib.fill_stream_run(self.handle, e, seed, reg.ctypes.data, threshold, 0, None, None, None, None))
        seg, acc = np.full((n + 1, 4), 77.0, f32), np.full(n + 1, 77, np.uint32)
        col = None if rgba is None else np.ascontiguousarray(rgba, f32)
        prims = None if rgba is None else np.zeros((n + 1, 20), np.uint32)
        again = int(self.lib.fill_stream_run(self.handle, e, seed, reg.ctypes.data, threshold, n, seg.ctypes.data, acc.ctypes.data,
                                             None if prims is None else prims.ctypes.data, None if col is None else col.ctypes.data))
        assert again == n and (seg[n] == 77.0).all() and acc[n] == 77
        out = {"segments": seg[:n], "accumulation": acc[:n], "total": n}
        if prims is not None:
            out["prims"] = prims[:n]
        return out


def extra_cases(tile):
    """name -> (dem, spacing or None, exaggeration): what the fill tests add to drainage_cases.named_cases()."""
    return {
        "pit": (pit(), None, 1.0),
        "nested": (nested(), None, 1.0),
        "relief 65x130": (relief((65, 130), 11), (10.0, 7.0), 1.0),
        "walled serpentine 35x35": (walled_serpentine(33), (10.0, 10.0), 1.0),
        # (a step of 1/16: the longer channel stays below its walls)
        f"walled serpentine {2 * tile + 3}": (walled_serpentine(2 * tile + 1, step=0.0625), (10.0, 10.0), 1.0),
    }
