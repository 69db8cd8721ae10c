#!/usr/bin/env python3
"""Writes tests/golden/eval_a.npz: the ragged batch of tests/_eval.py (CASES), unpadded, with

  x{b}, y{b}             the feature frames, float64 [Tx_b, D] and [Ty_b, D]
  total, total32         float64 [B]: the DTW total of (x, y) and of their float32 roundings
  K, K32                 int32 [B]: the path lengths
  pi{b}, pj{b}           int32 [K_b]: the path; pi32_{b}, pj32_{b}: of the float32 roundings
  total_rowwise          float64 [B]: the same recursion written a second time, cell by cell in row
                         order with Python floats and min(), NOT the restatement
  mel                    log-mel frames, float64 [40, 80], uniform in [-11.5, 2]
  dct_scipy              scipy.fft.dct(mel, type=2, norm="ortho", axis=1)[:, 1:14], NOT the restatement

The totals and paths come from the numpy restatement (tests/_eval.py: dtw_ref), which
test_eval_host.py holds against a brute-force enumeration of every warping path.

    python tests/golden/gen_golden_eval.py
"""
import os
import sys

import numpy as np
import scipy.fft

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _eval as E  # noqa: E402


def total_rowwise(c):
    Tx, Ty = c.shape
    A = [[float("inf")] * (Ty + 1) for _ in range(Tx + 1)]
    for i in range(Tx):
        for j in range(Ty):
            best = 0.0 if i == 0 and j == 0 else min(A[i][j], A[i][j + 1], A[i + 1][j])
            A[i + 1][j + 1] = float(c[i, j]) + best
    return A[Tx][Ty]


def main():
    _, _, xs, ys = E.batch_feats(np.float64)
    out = {"cases": np.array(E.CASES, dtype=np.int64)}
    tot, tot32, Ks, Ks32, rowwise = [], [], [], [], []
    for b, (x, y) in enumerate(zip(xs, ys)):
        out[f"x{b}"], out[f"y{b}"] = x, y
        t, K, pi, pj = E.dtw_ref(x, y)
        out[f"pi{b}"], out[f"pj{b}"] = pi, pj
        tot.append(t)
        Ks.append(K)
        rowwise.append(total_rowwise(E.pair_dist_ref(x, y)))
        t, K, pi, pj = E.dtw_ref(x.astype(np.float32), y.astype(np.float32))
        out[f"pi32_{b}"], out[f"pj32_{b}"] = pi, pj
        tot32.append(t)
        Ks32.append(K)
    out.update(total=np.array(tot), total32=np.array(tot32), K=np.array(Ks, dtype=np.int32),
               K32=np.array(Ks32, dtype=np.int32), total_rowwise=np.array(rowwise))
    mel = E.make_mel(40, 77)
    out["mel"] = mel
    out["dct_scipy"] = scipy.fft.dct(mel, type=2, norm="ortho", axis=1)[:, 1:E.N_COEF + 1]
    np.savez_compressed(E.GOLDEN, **out)
    print(f"wrote {E.GOLDEN}: {os.path.getsize(E.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
