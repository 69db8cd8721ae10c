#!/usr/bin/env python3
"""Writes tests/golden/align_a.npz: the ragged batch of tests/_align.py (CASES), unpadded, with

  x{b}                 the attention log-probabilities, float64 [T_b, L_b]
  dur{b}, path{b}      the monotonic alignment of x{b}; dur32_{b}, path32_{b}: of its float32 rounding
  score, score32       float64 [B]
  nll, nll32           float64 [B]: torch's CPU float64 ctc_loss of log_softmax([blank, x]) with the
                       targets 1..L_b (reduction "sum", zero_infinity), for x and its float32 rounding
  grad{b}, grad32_{b}  d nll_b / d x from torch.autograd through the same expression

The alignment comes from the numpy restatement (tests/_align.py: mas_ref), which test_align_host.py
holds against a brute-force enumeration; nll and the gradients come from torch, NOT from the
restatement, which the same test file compares with them.

    python tests/golden/gen_golden_align.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _align as A  # noqa: E402


def torch_ctc(x, blank=A.BLANK):
    """(nll, d nll / d x) of one utterance, float64 on the CPU."""
    x = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    T, L = x.shape
    z = torch.cat([torch.full((T, 1), blank, dtype=torch.float64), x], dim=1)
    lp = F.log_softmax(z, dim=1)
    nll = F.ctc_loss(lp[:, None, :], torch.arange(1, L + 1)[None], [T], [L], reduction="sum", zero_infinity=True)
    nll.backward()
    return float(nll.detach()), x.grad.numpy().copy()


def main():
    _, mats = A.batch_logp(np.float64)
    out = {"cases": np.array(A.CASES, dtype=np.int64), "blank": np.float64(A.BLANK)}
    for tag, cast in (("", np.float64), ("32", np.float32)):
        sep = "_" if tag else ""
        scores, nlls = [], []
        for b, m in enumerate(mats):
            x = m.astype(cast)
            dur, score, path = A.mas_ref(x)
            nll, grad = torch_ctc(x)
            out[f"dur{tag}{sep}{b}"], out[f"path{tag}{sep}{b}"], out[f"grad{tag}{sep}{b}"] = dur, path, grad
            scores.append(score)
            nlls.append(nll)
            if not tag:
                out[f"x{b}"] = m
        out[f"score{tag}"], out[f"nll{tag}"] = np.array(scores), np.array(nlls)
    np.savez_compressed(A.GOLDEN, **out)
    print(f"wrote {A.GOLDEN}: {os.path.getsize(A.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
