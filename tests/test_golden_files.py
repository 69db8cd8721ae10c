"""The fixture store itself: every file under tests/golden/ within the size limit for a committed
file, and the part-wise npz writer / reader (tests/_npz_parts.py) exact."""
import os

import numpy as np

from _common import GOLDEN
from _npz_parts import load_npz_parts, save_npz_parts


def test_no_golden_file_above_one_mib():
    big = {}
    for root, _, files in os.walk(GOLDEN):
        for f in files:
            n = os.path.getsize(os.path.join(root, f))
            if n > 1 << 20:
                big[os.path.relpath(os.path.join(root, f), GOLDEN)] = n
    assert not big, big


def test_npz_parts_round_trip(tmp_path, monkeypatch):
    import _npz_parts

    monkeypatch.setattr(_npz_parts, "PART_LIMIT", 20000)
    rng = np.random.default_rng(0)
    arrays = {"mels": rng.standard_normal((2, 97, 80)).astype(np.float32),  # ~57 kB packed: cut into pieces
              "ids": rng.integers(0, 100, (3, 7)), "scalar": np.array(5), "names": np.array(["a", "bc"]),
              "wide": rng.standard_normal((1, 3000)).astype(np.float32)}  # cannot be cut along its first axis
    path = str(tmp_path / "case.npz")
    n = save_npz_parts(path, **arrays)
    assert n > 1 and all(os.path.getsize(os.path.join(tmp_path, f)) <= 20000 for f in os.listdir(tmp_path))
    z = load_npz_parts(path)
    assert z.files == list(arrays)
    for k, v in arrays.items():
        assert z[k].dtype == v.dtype and z[k].shape == v.shape
        np.testing.assert_array_equal(z[k], v)
    # a later, smaller version leaves no stale part behind
    assert save_npz_parts(path, ids=arrays["ids"]) == 1
    assert os.listdir(tmp_path) == ["case.npz"] and load_npz_parts(path).files == ["ids"]
