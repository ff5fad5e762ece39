"""An independent statement of the fill contract (csrc/f3d_fill.h) -- TEST INFRASTRUCTURE ONLY.

NumPy and heapq, sample by sample; it knows nothing of tiles, rounds or path doubling:
* the filled surface W: a priority-flood from the border with a heap;
* the flat distance T: a queue BFS per plateau of W, from the samples with a strictly lower neighbour and the outlets;
* directions: drainage_reference.slopes on W, then, for an interior sample without a positive slope, the lowest code with a
  smaller W or an equal W and a smaller T;
* accumulation: the samples visited in descending (W, T), each handing its count to its receiver;
* streams: drainage_reference.streams over that routing.
"""
from __future__ import annotations

import heapq
from collections import deque

import numpy as np

import drainage_reference as ref

f32 = np.float32
FAR = 0xFFFFFFFF


def outlets(shape):
    """bool (H, W): the first and last row and column."""
    out = np.zeros(shape, bool)
    out[0, :] = out[-1, :] = out[:, 0] = out[:, -1] = True
    return out


def _neighbours(j, i, rows, cols):
    for k, (dj, di) in enumerate(ref.STEPS):
        nj, ni = j + dj, i + di
        if 0 <= nj < rows and 0 <= ni < cols:
            yield k, nj, ni


def filled_surface(heights):
    """float32 (H, W): priority-flood.  Every border sample enters the heap at its own height; a sample popped at level L gives
    each unvisited neighbour the level max(its height, L)."""
    z = np.asarray(heights, f32)
    rows, cols = z.shape
    W = np.full(z.shape, np.inf, f32)
    done = np.zeros(z.shape, bool)
    heap = []
    for j, i in zip(*np.nonzero(outlets(z.shape))):
        W[j, i] = z[j, i]
        done[j, i] = True
        heap.append((float(z[j, i]), int(j), int(i)))
    heapq.heapify(heap)
    while heap:
        level, j, i = heapq.heappop(heap)
        for _, nj, ni in _neighbours(j, i, rows, cols):
            if not done[nj, ni]:
                done[nj, ni] = True
                W[nj, ni] = max(z[nj, ni], f32(level))
                heapq.heappush(heap, (float(W[nj, ni]), nj, ni))
    return W


def flat_distance(W):
    """uint32 (H, W): 0 on outlets and where a neighbour is strictly lower; elsewhere the BFS distance to such a sample through
    neighbours of equal W."""
    rows, cols = W.shape
    T = np.full(W.shape, FAR, np.uint32)
    queue = deque()
    border = outlets(W.shape)
    for j in range(rows):
        for i in range(cols):
            if border[j, i] or any(W[nj, ni] < W[j, i] for _, nj, ni in _neighbours(j, i, rows, cols)):
                T[j, i] = 0
                queue.append((j, i))
    while queue:
        j, i = queue.popleft()
        for _, nj, ni in _neighbours(j, i, rows, cols):
            if T[nj, ni] == FAR and W[nj, ni] == W[j, i]:
                T[nj, ni] = T[j, i] + 1
                queue.append((nj, ni))
    return T


def directions(W, T, spacing):
    s = ref.slopes(W, spacing)
    rows, cols = W.shape
    border = outlets(W.shape)
    code = np.full(W.shape, ref.SINK, np.uint8)
    for j in range(rows):
        for i in range(cols):
            best = f32(0.0)
            for k in range(8):
                v = s[k, j, i]
                if v > best:
                    best, code[j, i] = v, k
            if code[j, i] != ref.SINK or border[j, i]:
                continue
            for k, nj, ni in _neighbours(j, i, rows, cols):
                if W[nj, ni] < W[j, i] or (W[nj, ni] == W[j, i] and T[nj, ni] < T[j, i]):
                    code[j, i] = k
                    break
            assert code[j, i] != ref.SINK, "the last rule always finds a neighbour"
    return code


def route(heights, spacing):
    """{"filled", "depth" float32, "flat_distance" uint32, "direction" uint8, "accumulation", "basin" uint32 (H, W), "sinks",
    "longest", "filled_samples", "largest_flat_distance"} of the whole DEM."""
    z = (np.asarray(heights, f32) + f32(0.0)).astype(f32)  # (-0 becomes +0: equal values have equal bits)
    W = filled_surface(z)
    T = flat_distance(W)
    assert (T != FAR).all(), "every sample gets a finite T"
    code = directions(W, T, spacing)
    recv = ref.receivers(code)
    n = z.size
    sink = code.reshape(-1) == ref.SINK
    key = list(zip(W.reshape(-1).tolist(), T.reshape(-1).tolist()))
    assert all(key[recv[v]] < key[v] for v in range(n) if not sink[v]), "every step lowers (W, T)"
    order = sorted(range(n), key=lambda v: key[v], reverse=True)  # descending: every sample before its receiver
    acc = np.ones(n, np.int64)
    for v in order:
        if not sink[v]:
            acc[recv[v]] += acc[v]
    basin = np.full(n, -1, np.int64)
    depth = np.zeros(n, np.int64)
    for v in order[::-1]:
        basin[v] = v if sink[v] else basin[recv[v]]
        depth[v] = 0 if sink[v] else depth[recv[v]] + 1
    return {"filled": W, "depth": (W - z).astype(f32), "flat_distance": T, "direction": code,
            "accumulation": acc.astype(np.uint32).reshape(z.shape), "basin": basin.astype(np.uint32).reshape(z.shape),
            "sinks": int(sink.sum()), "longest": int(depth.max()), "filled_samples": int((W > z).sum()), "largest_flat_distance": int(T.max())}
