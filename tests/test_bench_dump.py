"""bench.py --dump-outputs on CPU tensors: what sample() returned is written whole as float32
.npy files when it fits the byte limit, and as the same seeded, ascending choice of rows from
every array when it does not, identically from run to run."""
import os

import numpy as np
import torch

import bench


def _result(rows, with_start=True):
    img = torch.arange(rows * 4 * 8, dtype=torch.float32).reshape(rows, 4, 8)
    return img, (-img if with_start else None)


def test_small_result_is_written_whole(tmp_path):
    img, start = _result(10)
    bench.dump_outputs(str(tmp_path / "d"), (img, start))
    assert sorted(os.listdir(tmp_path / "d")) == ["latents.npy", "start_noise.npy"]
    a = np.load(tmp_path / "d" / "latents.npy")
    assert a.dtype == np.float32
    np.testing.assert_array_equal(a, img.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "start_noise.npy"), start.numpy())


def test_missing_start_noise_is_left_out(tmp_path):
    bench.dump_outputs(str(tmp_path), _result(3, with_start=False))
    assert os.listdir(tmp_path) == ["latents.npy"]


def test_large_result_is_sampled_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)  # 2 arrays x 128 B per row -> 16 rows
    img, start = _result(100)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), (img, start))
    a, s = np.load(tmp_path / "a" / "latents.npy"), np.load(tmp_path / "a" / "start_noise.npy")
    assert a.shape == s.shape == (16, 4, 8) and a.nbytes + s.nbytes <= 4096
    np.testing.assert_array_equal(s, -a)                     # the same rows of both arrays
    rows = (a[:, 0, 0] / 32).astype(int)
    assert (np.diff(rows) > 0).all() and rows.max() < 100
    np.testing.assert_array_equal(a, img.numpy()[rows])      # whole rows of the original
    np.testing.assert_array_equal(a, np.load(tmp_path / "b" / "latents.npy"))
