"""`-m gpu`: the library's process-wide device state between two calls, and the call after it.

Every kernel of the library is compared with an oracle elsewhere, one call at a time.  What those tests never do is change
the state that outlives a call before the next one: the smoke workspace (per sequence handle and per stream, f3d_devmem.h),
the device pool that f3d_device_pool_trim empties (the strip driver calls it by itself, forge3d_amd/distributed.py), and
the scene and mesh caches that f3d_scene_cache_limit evicts while sessions still hold their entries (f3d_host_mem.h).
Here each of those changes happens between two calls, and the image after it is compared byte for byte with the CPU
oracle and with an undisturbed twin:
  * smoke sequences with a trim after a render, between every frame, and before close();
  * the handle-less smoke entry points, whose workspace grows from a small image to 1080p and is then reused larger;
  * terrain sessions whose DEM tables and mesh are evicted while they live, with both mesh builders, with and without trims;
  * four threads that create sessions over one DEM and one mesh at the same moment (the mesh cache's insert);
  * the smoke-sequence and eviction cases again in a child process per poison pattern (f3d_debug_poison).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

import scenes
from oracle import smoke_oracle as so

pytestmark = pytest.mark.gpu

# the library's scene-cache limit when a test starts (f3d_host_mem.h g_scene_limit; the ABI has no getter, and every test of
# the suite that changes it puts this value back)
CACHE_LIMIT = 2

# ---- the smoke sequence: a small plume over a random terrain frame, self-shadowing on (the deferred shadow list) ----
SMOKE_DIMS = (24, 16, 20)
SMOKE_W, SMOKE_H = 160, 96
SMOKE_FRAMES = 5
SMOKE_STEPS = 2
SMOKE_CAM = dict(camera_pos=(12.0, 10.0, 46.0), target=(12.0, 6.0, 10.0))
SMOKE_EMITTERS = [dict(center=(6.0, 3.0, 10.0), radius=2.5, density_rate=6.0, temperature_rate=3.0, soot_rate=0.3, emission_rate=2.0,
                       velocity=(3.0, 0.4, 0.0))]
SMOKE_SETTINGS = dict(dt=0.1, turbulence_strength=0.5, turbulence_seed=7, wind=(1.5, 0.0, -0.2), pressure_iterations=8)
NO_SCRATCH = {"scratch_bytes": 0, "shadow_list_chunks": 0, "shadow_list_chunks_used": 0, "shadow_list_slots_per_chunk": 1024}

# ---- the terrain sessions: the golden DEM with a box city, 2 frames a render ----
TERRAIN_W, TERRAIN_H = 96, 72
TERRAIN_FRAMES = 6
TERRAIN_STEP = 2
BUILDERS = {1: "host BVH", 2: "GPU LBVH"}
AOVS = ("rgba", "albedo", "normal", "depth")


def _lib():
    from forge3d_amd import _native

    return _native.lib()


def _trim():
    _lib().f3d_device_pool_trim()


@contextlib.contextmanager
def _cache_limit_restored():
    try:
        yield
    finally:
        _lib().f3d_scene_cache_limit(C.c_uint32(CACHE_LIMIT))


def _smoke_terrain():
    rng = np.random.default_rng(3)
    terrain = rng.integers(0, 256, (SMOKE_H, SMOKE_W, 4), dtype=np.uint8)
    terrain[..., 3] = 255
    return terrain


def _smoke_oracle_frames(count):
    """The oracle's frames of the sequence: steps -> march -> atmospheric composite over the terrain frame."""
    terrain, st, out = _smoke_terrain(), so.new_state(SMOKE_DIMS), []
    for _ in range(count):
        so.step(st, SMOKE_EMITTERS, steps=SMOKE_STEPS, **SMOKE_SETTINGS)
        fields = {k: st[k] for k in ("density", "temperature", "soot", "humidity", "emission_rate", "particle_age")}
        out.append(so.composite_atmospheric(terrain, so.render_rgba(fields, SMOKE_W, SMOKE_H, frame_index=st["frame_index"], **SMOKE_CAM)))
    return out


def _terrain_scene():
    dem = scenes.golden_dem()
    v, i = scenes.box_city(40)
    kw = scenes.fixed_frames(scenes.scene_kwargs(dem), TERRAIN_FRAMES, spp=2, mesh_vertices=v, mesh_indices=i)
    return dem, kw


@pytest.fixture(scope="module")
def smoke_want():
    want = _smoke_oracle_frames(SMOKE_FRAMES)
    assert int(want[-1][..., 3].min()) == 255 and not np.array_equal(want[0], want[-1])  # the plume moves
    return want


@pytest.fixture(scope="module")
def terrain_want():
    """The oracle's image after 2, 4 and 6 frames (one oracle render each: the accumulation of frames 0..k-1)."""
    from oracle import oracle

    dem, kw = _terrain_scene()
    want = {k: oracle.render(dem, TERRAIN_W, TERRAIN_H, scenes.CAM, **dict(kw, max_frames=k, min_frames=k))
            for k in range(TERRAIN_STEP, TERRAIN_FRAMES + 1, TERRAIN_STEP)}
    assert np.isclose(want[TERRAIN_FRAMES]["albedo"][..., 2], 0.8, atol=2e-3).any()  # the boxes are in view (mesh albedo 0.7, 0.7, 0.8)
    return want


def _same_frames(got, want, what):
    assert len(got) == len(want), what
    for f, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (what, f)
        assert np.array_equal(a, b), f"{what}: frame {f} differs in {int(np.any(a != b, axis=-1).sum())} pixels"


def _same_image(got, want, what):
    for key in AOVS:
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{what}: {key} differs"


# ------------------------------------------------------------------------------------------------------------------------
# smoke sequence (f3d_smoke_seq_*) against f3d_device_pool_trim
# ------------------------------------------------------------------------------------------------------------------------
def _sequence():
    from forge3d_amd import smoke

    return smoke.SmokeSequence(smoke.SmokeDomain(SMOKE_DIMS), _smoke_terrain(), **SMOKE_CAM)


def _frames(seq, count, overlap, between=None):
    """`count` frames of `seq` (copies); between(i) runs in the loop body after frame i arrived, while frame i + 1 is enqueued."""
    from forge3d_amd import smoke

    settings = smoke.SmokeStepSettings(**SMOKE_SETTINGS)
    emitters = [smoke.SmokeEmitter(**e) for e in SMOKE_EMITTERS]
    out = []
    for i, frame in enumerate(seq.frames(count, settings, emitters, steps_per_frame=SMOKE_STEPS, overlap=overlap)):
        out.append(frame.copy())
        if between is not None:
            between(i)
    return out


def _smoke_trim_run(overlap):
    """A sequence with a trim between every two frames beside its undisturbed twin.  Returns the frames of both, the stats()
    of both in the loop body of every frame but the last (there the frame after it has just been rendered), and the
    trimmed sequence's stats() after its last trim."""
    twin, twin_stats = _sequence(), []
    twin_frames = _frames(twin, SMOKE_FRAMES, overlap, lambda i: twin_stats.append(twin.stats()) if i + 1 < SMOKE_FRAMES else None)
    twin.close()
    seq, stats = _sequence(), []

    def stats_then_trim(i):
        if i + 1 < SMOKE_FRAMES:
            stats.append(seq.stats())
        _trim()

    frames = _frames(seq, SMOKE_FRAMES, overlap, stats_then_trim)
    after = seq.stats()
    seq.close()
    return frames, twin_frames, stats, twin_stats, after


@pytest.mark.parametrize("overlap", [True, False])
def test_sequence_stats_after_a_trim_report_no_scratch_and_no_shadow_list(smoke_want, overlap):
    """render -> f3d_device_pool_trim -> stats: the trim freed the sequence's scratch, the self-shadow list with it, and
    stats() says so (it used to read the list's fill count from the freed buffer).  The sequence renders on after it."""
    seq = _sequence()
    first = _frames(seq, SMOKE_FRAMES - 2, overlap)
    _same_frames(first, smoke_want[:SMOKE_FRAMES - 2], "before the trim")
    before = seq.stats()
    assert before["scratch_bytes"] > 0 and 0 < before["shadow_list_chunks_used"] <= before["shadow_list_chunks"]
    _trim()
    assert seq.stats() == NO_SCRATCH
    assert seq.stats() == NO_SCRATCH  # (asking twice changes nothing)
    rest = _frames(seq, 2, overlap)
    _same_frames(rest, smoke_want[SMOKE_FRAMES - 2:], "after the trim")
    again = seq.stats()  # the next render allocated the same scratch and a list of the same capacity, and filled it
    assert (again["scratch_bytes"], again["shadow_list_chunks"]) == (before["scratch_bytes"], before["shadow_list_chunks"])
    assert 0 < again["shadow_list_chunks_used"] <= again["shadow_list_chunks"]
    seq.close()


@pytest.mark.parametrize("overlap", [True, False])
def test_sequence_with_a_trim_between_every_frame_equals_its_twin_and_the_oracle(smoke_want, overlap):
    """f3d_device_pool_trim between every two frames (while the next frame is in flight): every frame is the oracle's and the
    untrimmed twin's, and stats() after each render that followed a trim is the twin's at the same frame."""
    frames, twin_frames, stats, twin_stats, after = _smoke_trim_run(overlap)
    _same_frames(twin_frames, smoke_want, "twin")
    _same_frames(frames, smoke_want, "trimmed")
    _same_frames(frames, twin_frames, "trimmed against the twin")
    assert len(stats) == SMOKE_FRAMES - 1 and stats == twin_stats
    assert all(s["scratch_bytes"] > 0 and 0 < s["shadow_list_chunks_used"] <= s["shadow_list_chunks"] for s in stats)
    assert after == NO_SCRATCH  # (the last frame's render came before the last trim)


@pytest.mark.parametrize("overlap", [True, False])
def test_close_after_a_trim_and_a_fresh_handle_give_the_frames_again(smoke_want, overlap):
    """close() of a sequence whose scratch a trim already freed returns cleanly (its handles release nothing twice), and a
    fresh sequence renders the oracle's frames again -- also the first time after a trim emptied the pool."""
    seq = _sequence()
    first = _frames(seq, SMOKE_FRAMES, overlap)
    _trim()
    seq.close()
    assert seq._handles == {}
    seq.close()
    _trim()
    again = _sequence()
    second = _frames(again, SMOKE_FRAMES, overlap)
    again.close()
    _same_frames(first, smoke_want, "first sequence")
    _same_frames(second, smoke_want, "fresh sequence")


# ------------------------------------------------------------------------------------------------------------------------
# handle-less smoke calls (f3d_smoke_step / _render / _composite on the thread's default context): workspace regrowth
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim", [False, True])
def test_handle_less_smoke_calls_regrow_and_reuse_their_workspace(trim):
    """One thread, the null stream: a step, a march and a composite at 160x96, then at 1920x1080 (the workspace grows: larger
    records, image and shadow list), then at 160x96 again (the 1080p buffers are reused, larger than needed) -- each the
    oracle's, with or without a trim between the calls."""
    from forge3d_amd import smoke

    dom, st = smoke.SmokeDomain(SMOKE_DIMS), so.new_state(SMOKE_DIMS)
    settings, emitters = smoke.SmokeStepSettings(**SMOKE_SETTINGS), [smoke.SmokeEmitter(**e) for e in SMOKE_EMITTERS]
    rng = np.random.default_rng(5)
    for call, (w, h) in enumerate([(160, 96), (1920, 1080), (160, 96), (96, 160)]):
        dom.step(settings, emitters, steps=SMOKE_STEPS + call)
        so.step(st, SMOKE_EMITTERS, steps=SMOKE_STEPS + call, **SMOKE_SETTINGS)
        assert np.array_equal(dom.density, st["density"]) and np.array_equal(dom.velocity, st["velocity"]), call
        if trim:
            _trim()
        layer = dom.render_rgba(w, h, **SMOKE_CAM)
        fields = {k: st[k] for k in ("density", "temperature", "soot", "humidity", "emission_rate", "particle_age")}
        want = so.render_rgba(fields, w, h, frame_index=st["frame_index"], **SMOKE_CAM)
        assert layer.shape == (h, w, 4) and np.array_equal(layer, want), f"march {w}x{h} (call {call}) differs in {int(np.any(layer != want, -1).sum())} pixels"
        assert int(want[..., 3].max()) > 40, call  # the plume is in the picture
        if trim:
            _trim()
        base = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        base[..., 3] = 255
        assert np.array_equal(smoke.composite_atmospheric_smoke(base, layer), so.composite_atmospheric(base, want)), f"composite {w}x{h}"


# ------------------------------------------------------------------------------------------------------------------------
# terrain sessions against eviction from the scene and mesh caches
# ------------------------------------------------------------------------------------------------------------------------
class _Renders:
    """A session rendered TERRAIN_STEP frames at a time: each render continues the accumulation and resolves it."""

    def __init__(self, dem, kw, builder):
        from forge3d_amd.session import TerrainSession

        self.session = TerrainSession(dem, TERRAIN_W, TERRAIN_H, scenes.CAM, mesh_builder=builder, **kw)
        self.done = 0

    def render(self):
        self.session.enqueue_frames(self.done, TERRAIN_STEP)
        self.done += TERRAIN_STEP
        return self.done, self.session.resolve(self.done)

    def close(self):
        self.session.close()


def _eviction_run(builder, trim):
    """Session A lives while f3d_scene_cache_limit(0) evicts its DEM tables and mesh; session B is created over the same DEM
    and mesh after that; A and B render in turns, A goes, B renders on.  Returns [(label, frames, image)] in render order
    and the undisturbed twin's {frames: image}."""
    dem, kw = _terrain_scene()
    with _cache_limit_restored():
        twin = _Renders(dem, kw, builder)
        twin_images = dict(twin.render() for _ in range(TERRAIN_FRAMES // TERRAIN_STEP))
        twin.close()
        a = _Renders(dem, kw, builder)
        _lib().f3d_scene_cache_limit(C.c_uint32(0))  # A's tables and mesh leave both caches; A still holds them
        assert _lib().f3d_scene_cache_entries() == 0
        _lib().f3d_scene_cache_limit(C.c_uint32(CACHE_LIMIT))
        b = _Renders(dem, kw, builder)  # builds its own
        out = []
        for _ in range(2):
            out.append(("A",) + a.render())
            if trim:
                _trim()
            out.append(("B",) + b.render())
            if trim:
                _trim()
        a.close()
        if trim:
            _trim()  # (what A held is in the pool now: out to the driver)
        out.append(("B",) + b.render())
        b.close()
    return out, twin_images


@pytest.mark.parametrize("trim", [False, True], ids=["no_trim", "trim"])
@pytest.mark.parametrize("builder", sorted(BUILDERS), ids=lambda b: BUILDERS[b].replace(" ", "_"))
def test_sessions_survive_the_eviction_of_their_tables_and_mesh(terrain_want, builder, trim):
    """A live session keeps what the caches dropped, a session created after the eviction builds its own, and the two render
    in turns (with a trim between every two renders, or not): every image is the oracle's and the twin's."""
    out, twin = _eviction_run(builder, trim)
    assert [(label, frames) for label, frames, _ in out] == [("A", 2), ("B", 2), ("A", 4), ("B", 4), ("B", 6)]
    assert sorted(twin) == sorted(terrain_want)
    for frames, image in twin.items():
        _same_image(image, terrain_want[frames], f"twin after {frames} frames")
    for label, frames, image in out:
        what = f"{BUILDERS[builder]}, session {label} after {frames} frames"
        _same_image(image, terrain_want[frames], what)
        _same_image(image, twin[frames], what + " (twin)")


@pytest.mark.parametrize("builder", sorted(BUILDERS), ids=lambda b: BUILDERS[b].replace(" ", "_"))
def test_sessions_created_by_four_threads_at_once_render_the_oracle_image(terrain_want, builder):
    """Four threads create sessions over one DEM and one mesh at the same moment (ctypes lets go of the GIL), into emptied
    caches: all of them miss, build, and insert (f3d_host_mem.h acquire_mesh looks again under the lock).  Every image is
    the oracle's and no call raises; a session created after them finds the mesh cached and renders the same image."""
    from forge3d_amd.session import TerrainSession

    dem, kw = _terrain_scene()
    n = 4
    start = threading.Barrier(n)
    images, errors = [None] * n, []

    def work(k):
        try:
            start.wait(timeout=120)
            with TerrainSession(dem, TERRAIN_W, TERRAIN_H, scenes.CAM, mesh_builder=builder, **kw) as s:
                s.enqueue_frames(0, TERRAIN_STEP)
                images[k] = s.resolve(TERRAIN_STEP)
        except BaseException as exc:  # noqa: BLE001 -- reported below
            errors.append(exc)

    with _cache_limit_restored():
        _lib().f3d_scene_cache_limit(C.c_uint32(0))  # empty...
        _lib().f3d_scene_cache_limit(C.c_uint32(CACHE_LIMIT))  # ...and on again
        threads = [threading.Thread(target=work, args=(k,)) for k in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(600)
        assert not any(t.is_alive() for t in threads), "a session creation did not return"
        assert not errors, errors
        after = _Renders(dem, kw, builder)
        _, later = after.render()
        after.close()
    for k, image in enumerate(images):
        _same_image(image, terrain_want[TERRAIN_STEP], f"{BUILDERS[builder]}, thread {k}")
    _same_image(later, terrain_want[TERRAIN_STEP], f"{BUILDERS[builder]}, the session after the threads")


# ------------------------------------------------------------------------------------------------------------------------
# the same under poison (every device buffer and its guard regions filled with a pattern), a process per pattern
# ------------------------------------------------------------------------------------------------------------------------
def _lifecycle_outputs():
    """The images of the smoke-sequence and eviction cases, by name."""
    out = {}
    for overlap in (True, False):
        frames, twin_frames, stats, twin_stats, after = _smoke_trim_run(overlap)
        assert stats == twin_stats and after == NO_SCRATCH, overlap
        for f, (a, b) in enumerate(zip(frames, twin_frames)):
            out[f"smoke_overlap{int(overlap)}_f{f}"] = a
            out[f"smoke_overlap{int(overlap)}_twin_f{f}"] = b
    for builder in sorted(BUILDERS):
        for trim in (False, True):
            images, twin = _eviction_run(builder, trim)
            for n, (label, frames, image) in enumerate(images + [("twin", k, v) for k, v in sorted(twin.items())]):
                for key in AOVS:
                    out[f"terrain_b{builder}_t{int(trim)}_{n}_{label}{frames}_{key}"] = image[key]
    return out


def _poisoned_lifecycle_case(pattern, path):
    """Body of test_poisoned_lifecycle_cases_equal_the_unpoisoned_ones, in a process of its own (the pattern stays there)."""
    from forge3d_amd import _native

    _native.debug_poison(pattern)
    np.savez(path, **_lifecycle_outputs())


@pytest.mark.parametrize("pattern", [0xFF, 0x5A])
def test_poisoned_lifecycle_cases_equal_the_unpoisoned_ones(smoke_want, terrain_want, tmp_path, pattern):
    """Poison mode (f3d_debug_poison): every buffer allocated after a trim or an eviction starts as the pattern.  The
    smoke-sequence and eviction cases in a child process under the pattern give the unpoisoned outputs, which are the
    oracle's -- nothing reads memory that the call before it left behind."""
    import multiprocessing as mp

    path = tmp_path / "poisoned.npz"
    proc = mp.get_context("spawn").Process(target=_poisoned_lifecycle_case, args=(pattern, str(path)))
    proc.start()
    proc.join(600)
    if proc.is_alive():
        proc.kill()
        proc.join()
    assert proc.exitcode == 0
    want = _lifecycle_outputs()
    with np.load(path) as got:
        assert sorted(got.files) == sorted(want)
        for name in want:
            assert np.array_equal(got[name], want[name], equal_nan=True), name
    for overlap in (0, 1):
        _same_frames([want[f"smoke_overlap{overlap}_f{f}"] for f in range(SMOKE_FRAMES)], smoke_want, f"overlap={overlap}")
    for name, value in want.items():
        if name.startswith("terrain_"):
            frames, key = int(name.split("_")[4].lstrip("ABtwin")), name.split("_")[-1]
            assert np.array_equal(value, terrain_want[frames][key], equal_nan=True), name
