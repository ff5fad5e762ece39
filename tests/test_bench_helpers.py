"""Host logic of bench.py that only an N > 1 run exercises on hardware: the one re-cut of the strips after the warm-up frames
 and the identity fields; the options of a plain run and what --dump-outputs writes.  No GPU."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


class _Renderer:
    def __init__(self, bounds, density=None):
        self.bounds, self.world, self.height = list(bounds), len(bounds) - 1, bounds[-1]
        if density is not None:
            self.cost_density = np.asarray(density, np.float64)
        self.closed = False

    def close(self):
        self.closed = True


def test_balanced_strips_are_left_alone():
    r = _Renderer([0, 400, 700, 1080])
    made = []
    got, report = bench.recut_after_warmup(r, [4.0, 4.1, 4.05], lambda b: made.append(b) or _Renderer(b))
    assert got is r and not r.closed and made == [] and report["recut"] is False and report["max_over_mean"] < 1.05


def test_an_imbalance_over_five_per_cent_recuts_once_towards_equal_cost():
    density = np.where(np.arange(1080) < 400, 0.2, 1.0)
    r = _Renderer([0, 360, 720, 1080], density)  # equal rows on a frame whose top is cheap sky
    times = [density[b0:b1].sum() / 100.0 for b0, b1 in zip(r.bounds, r.bounds[1:])]
    made = []
    got, report = bench.recut_after_warmup(r, times, lambda b: made.append(list(b)) or _Renderer(b, density))
    assert report["recut"] is True and r.closed and got is not r and made == [report["bounds_after"]]
    cost = [density[b0:b1].sum() for b0, b1 in zip(got.bounds, got.bounds[1:])]
    assert max(cost) / (sum(cost) / 3) < 1.03 and got.bounds[1] > 360  # the sky strip got fatter
    assert report["bounds_before"] == [0, 360, 720, 1080]


def test_a_new_cut_that_cannot_be_built_keeps_the_old_strips():
    r = _Renderer([0, 360, 720, 1080], np.where(np.arange(1080) < 400, 0.2, 1.0))

    def broken(bounds):
        raise RuntimeError("[Render] Render error: another rank of the strip job failed; this rank stops with it")

    got, report = bench.recut_after_warmup(r, [1.0, 3.0, 3.6], broken)
    assert got is r and not r.closed and report["recut"] is False and "another rank" in report["failed"]


def test_useless_times_never_recut():
    r = _Renderer([0, 540, 1080])
    for times in ([0.0, 1.0], [float("nan"), 1.0], [float("inf"), 1.0]):
        got, report = bench.recut_after_warmup(r, times, lambda b: (_ for _ in ()).throw(AssertionError("must not be called")))
        assert got is r and report["recut"] is False


def test_device_identity_reports_whatever_the_torch_build_exposes():
    class Props:
        name = "AMD Instinct MI355X"
        uuid = "abc"
        pci_bus_id = 5

    class Cuda:
        @staticmethod
        def get_device_properties(i):
            return Props()

    class Torch:
        cuda = Cuda()

    ident = bench.device_identity(Torch(), 3)
    assert ident == {"index": 3, "name": "AMD Instinct MI355X", "uuid": "abc", "pci_bus_id": "5"}


def _image(h, w, seed=0):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.0, 9.0, (h, w)).astype(np.float32)
    depth[0, :3] = np.nan  # sky: the renderer's miss marker
    return {"rgba": rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "albedo": rng.random((h, w, 3), np.float32),
            "normal": rng.random((h, w, 3), np.float32), "depth": depth, "any_valid_reservoir": True}


def test_dump_outputs_writes_the_image_as_finite_float32(tmp_path):
    img = _image(6, 10)
    bench.dump_outputs(tmp_path / "out", img)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["albedo.npy", "depth.npy", "hit.npy", "normal.npy", "rgba.npy"]
    for key in ("rgba", "albedo", "normal"):
        got = np.load(tmp_path / "out" / f"{key}.npy")
        assert got.dtype == np.float32 and got.shape == img[key].shape
        assert np.array_equal(got, img[key].astype(np.float32))
    depth, hit = np.load(tmp_path / "out" / "depth.npy"), np.load(tmp_path / "out" / "hit.npy")
    assert depth.dtype == hit.dtype == np.float32 and depth.shape == hit.shape == (6, 10)
    assert np.isfinite(depth).all() and set(np.unique(hit)) == {0.0, 1.0}
    sky = np.isnan(img["depth"])
    assert np.array_equal(hit == 0.0, sky) and (depth[sky] == 0.0).all() and np.array_equal(depth[~sky], img["depth"][~sky])


def test_dump_outputs_refuses_a_non_finite_value_it_cannot_explain(tmp_path):
    img = _image(4, 4)
    img["albedo"][1, 2, 0] = np.inf
    with pytest.raises(ValueError, match="albedo"):
        bench.dump_outputs(tmp_path / "out", img)
    assert not (tmp_path / "out").exists()


def test_dump_outputs_samples_the_same_pixels_when_the_image_is_too_large(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 48 * 100)  # 100 pixels of 12 float32 channels
    img = _image(20, 30, seed=1)
    bench.dump_outputs(tmp_path / "a", img)
    bench.dump_outputs(tmp_path / "b", _image(20, 30, seed=1))
    total = 0
    for key, chans in (("rgba", 4), ("albedo", 3), ("normal", 3), ("depth", 1), ("hit", 1)):
        a, b = np.load(tmp_path / "a" / f"{key}.npy"), np.load(tmp_path / "b" / f"{key}.npy")
        assert a.dtype == np.float32 and a.shape == (100, chans) and np.isfinite(a).all() and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_BYTES
    # the rows are pixels of the image, in raster order, the same pixels for every array
    first_albedo = img["albedo"][..., 0].reshape(-1)
    idx = [int(np.flatnonzero(first_albedo == v)[0]) for v in np.load(tmp_path / "a" / "albedo.npy")[:, 0]]
    assert idx == sorted(idx)
    assert np.array_equal(np.load(tmp_path / "a" / "rgba.npy"), img["rgba"].reshape(-1, 4)[idx].astype(np.float32))


def test_a_plain_run_is_the_default_and_steps_are_what_was_asked(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    args = bench.parse_args()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse_args()
    assert args.full and args.dump_outputs == "d" and args.steps == 32
