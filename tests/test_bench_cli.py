"""bench.py's command line on the host: the options of a plain / full run and the --dump-outputs writer."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_dtypes_and_names(tmp_path):
    g = torch.Generator().manual_seed(0)
    mel = torch.randn(2, 5, 80, generator=g).to(torch.bfloat16)
    mask = torch.tensor([[False, True], [True, True]])
    lens = torch.tensor([3, 5], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path), ["mel", "mel_masks", "mel_lens"], [mel, mask, lens])
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("mel", "mel_masks", "mel_lens")}
    assert got["mel"].dtype == np.float32 and got["mel"].shape == (2, 5, 80)
    np.testing.assert_array_equal(got["mel"], mel.float().numpy())
    assert got["mel_masks"].dtype == np.float32
    np.testing.assert_array_equal(got["mel_masks"], [[0, 1], [1, 1]])
    assert got["mel_lens"].dtype == np.float64
    np.testing.assert_array_equal(got["mel_lens"], [3, 5])
    bench.dump_outputs(str(tmp_path), ["mel"], [mel], rank=1)
    assert (tmp_path / "mel.rank1.npy").exists()


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    big = torch.arange(3000, dtype=torch.float32).reshape(30, 100)
    small = torch.arange(10, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "whole"), ["big", "small"], [big, small])
    np.testing.assert_array_equal(np.load(tmp_path / "whole" / "big.npy"), big.numpy())  # fits: not sampled
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)  # small takes 40 bytes, big the 3960 left = 990 float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ["big", "small"], [big, small])
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (990,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)  # the same sample every run
    assert np.all(np.diff(a) > 0) and a.max() < 3000  # distinct elements of the array, in order
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4000 + 2 * 128  # the .npy headers
