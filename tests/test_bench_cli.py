"""bench.py's command line and its --dump-outputs writer (host logic, no GPU)."""
import os

import numpy as np
import torch

import bench


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup) == (7, 2)
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    bench.dump_outputs(str(tmp_path), {"loss": torch.tensor([2.5]), "x": x})
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "x.npy"]
    got = np.load(tmp_path / "x.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert np.load(tmp_path / "loss.npy").tolist() == [2.5]


def test_dump_outputs_samples_under_the_cap(tmp_path):
    torch.manual_seed(0)
    big = torch.randn(5000)
    cap = 8192  # all files of the directory together, their headers included
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"loss": torch.tensor([1.0]), "params": big},
                           cap=cap)
    a, b = tmp_path / "a", tmp_path / "b"
    assert _dir_bytes(a) <= cap
    idx = np.load(a / "params_index.npy")
    assert idx.dtype == np.int64 and np.all(np.diff(idx) > 0) and idx[-1] < big.numel()
    assert np.array_equal(np.load(a / "params.npy"), big.numpy()[idx])
    # the sample is fixed: a second run picks the same positions
    assert np.array_equal(idx, np.load(b / "params_index.npy"))
    assert np.array_equal(np.load(a / "params.npy"), np.load(b / "params.npy"))
