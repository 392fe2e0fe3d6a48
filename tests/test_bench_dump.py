"""CPU: bench.py --dump-outputs -- what it writes, in which dtype, and that a large output is sampled the same way on every
run and stays under the byte budget."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_option_parses():
    assert bench.parse_args([]).dump_outputs is None
    assert bench.parse_args(["--dump-outputs", "out", "--steps", "7"]).dump_outputs == "out"


def test_small_output_is_written_whole_in_float32(tmp_path):
    img = torch.rand(12, 20, 3, generator=torch.Generator().manual_seed(0)).half()
    bench.dump_outputs(str(tmp_path), {"image": img})
    a = np.load(tmp_path / "image.npy")
    assert a.dtype == np.float32 and a.shape == (12, 20, 3)
    assert np.array_equal(a, img.float().numpy())


def test_large_output_is_a_fixed_sample_under_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 64_000)
    img = torch.arange(100 * 80 * 3, dtype=torch.float32).reshape(100, 80, 3)   # 96 000 bytes: over the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"image": img})
    a, b = np.load(tmp_path / "a" / "image_sample.npy"), np.load(tmp_path / "b" / "image_sample.npy")
    assert not os.path.exists(tmp_path / "a" / "image.npy")
    assert a.dtype == np.float32 and a.shape[1] == 3 and np.array_equal(a, b)
    assert os.path.getsize(tmp_path / "a" / "image_sample.npy") <= 64_000
    # every row is a whole pixel of the image, each pixel at most once, in image order
    rows = a[:, 0].astype(np.int64) // 3
    assert np.array_equal(a, img.reshape(-1, 3).numpy()[rows]) and np.all(np.diff(rows) > 0)
