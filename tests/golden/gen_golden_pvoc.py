#!/usr/bin/env python3
"""Write tests/golden/pvoc_a.npz: the outputs of the numpy restatement of include/fs2hip_pvoc.h
(tests/_pvoc.py) for the cases of _pvoc.fixture_cases(), nothing else. The inputs are generated from
seeds by the same module; a test checks that they still give these outputs.

    python tests/golden/gen_golden_pvoc.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _pvoc as V  # noqa: E402


def main():
    out = {}
    cases = V.fixture_cases()
    for name, (spec, T, rate) in cases.items():
        out["out_" + name] = V.pvoc(spec, T, rate)
        out["J_" + name] = np.int64(V.frames(T, rate))
    out["names"] = np.array(sorted(cases))
    path = os.path.join(HERE, "pvoc_a.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print(f"wrote {path}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
