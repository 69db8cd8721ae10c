#!/usr/bin/env python3
"""Write tests/golden/loudness_a.npz: the outputs of the numpy restatement of include/fs2hip_iir.h
(tests/_loudness.py) for the cases of _loudness.fixture_cases(), nothing else: per row the gated mean
square, the three block counts, and the gain, clipped count and first samples of its normalisation to
-23 LUFS; and the K-weighted output of one short row. The inputs are generated from seeds by the same
module; a test checks that they still give these outputs.

    python tests/golden/gen_golden_loudness.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _loudness as R  # noqa: E402


def main():
    out = {}
    cases = R.fixture_cases()
    for name, (x, fs) in cases.items():
        r = R.normalize(x, fs, -23.0)
        out["zbar_" + name] = np.float64(r["zbar"])
        out["counts_" + name] = np.array(r["counts"], dtype=np.int32)
        out["gain_" + name] = np.float64(r["gain"])
        out["clipped_" + name] = np.int32(r["clipped"])
        out["q_" + name] = r["q"][:2000]
    x, fs = cases["speech_i16_16000"]
    y, zf = R.sosfilt(x[:5000], R.k_weighting(fs))
    out["y_speech_i16_16000"], out["zf_speech_i16_16000"] = y, zf
    out["names"] = np.array(sorted(cases))
    path = os.path.join(HERE, "loudness_a.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print(f"wrote {path}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
