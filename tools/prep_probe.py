#!/usr/bin/env python3
"""Time the four preprocessing launches (include/fs2hip_prep.h) on a corpus-like batch, and the host
restatement of tests/_prep.py over the same arrays on the same machine.

    python tools/prep_probe.py [--reps 2000] [--rounds 5]

64 utterances of 860 frames and 64 phonemes: fs2_pitch_targets on the contours, then
fs2_outlier_moments, fs2_moments_merge and fs2_normalize_minmax on its phoneme-level targets, all
on device buffers allocated once (no host copy, no allocation in the timed loop). Each round is
event-timed over --reps passes after a warm-up, so a pass includes its five kernel launches'
enqueue cost. One JSON line per round, and one for the host.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def corpus_batch(B=64, T=860, Lx=64, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    f0 = np.zeros((B, T))
    dur = np.zeros((B, Lx), dtype=np.int64)
    for b in range(B):
        y = 180.0 + 40.0 * np.sin(t / 17.0 + rng.uniform(0, 6)) + 9.0 * np.sin(t / 3.1 + rng.uniform(0, 6))
        edges = np.sort(rng.choice(np.arange(5, T - 5), size=24, replace=False))
        for a, e in zip(edges[0::2], edges[1::2]):  # twelve voiced runs
            f0[b, a:e] = y[a:e]
        cuts = np.sort(rng.choice(np.arange(2, T), size=Lx - 1, replace=False))
        dur[b] = np.diff(np.concatenate([[0], cuts, [T]]))
    return f0, dur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from fs2amd import ops

    import _prep as P

    dev = torch.device("cuda:0")
    f0_h, dur_h = corpus_batch()
    B, T = f0_h.shape
    Lx = dur_h.shape[1]
    f0, dur = torch.from_numpy(f0_h).to(dev), torch.from_numpy(dur_h).to(dev)
    frames = torch.full((B,), T, dtype=torch.int64, device=dev)
    n_ph = torch.full((B,), Lx, dtype=torch.int64, device=dev)
    f64 = dict(device=dev, dtype=torch.float64)
    p_out = (torch.empty(B, Lx, **f64), torch.empty(B, T, **f64), torch.empty(B, device=dev, dtype=torch.int32))
    o_out = (torch.empty(B, 2, **f64), torch.empty(B, Lx, device=dev, dtype=torch.bool),
             torch.empty(B, device=dev, dtype=torch.int64), torch.empty(B, **f64), torch.empty(B, **f64))
    n_out = (torch.empty(B, Lx, **f64), torch.empty(2, **f64))
    ws = torch.empty(16 * B, device=dev, dtype=torch.uint8)
    state = torch.zeros(3, **f64)

    def one_pass():
        p = ops.pitch_targets(f0, dur, frames, out=p_out)
        o = ops.outlier_moments(p.out, n_ph, out=o_out)
        ops.moments_merge(state, o.count, o.mean, o.m2)
        ops.normalize_minmax(p.out, n_ph, mean=180.0, std=30.0, out=n_out, workspace=ws)

    for _ in range(20):
        one_pass()
    torch.cuda.synchronize(dev)
    for rnd in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            one_pass()
        e1.record()
        e1.synchronize()
        print(json.dumps({"round": rnd, "four_launches_us_per_pass": round(e0.elapsed_time(e1) * 1e3 / a.reps, 2),
                          "reps": a.reps, "utterances": B, "frames": T, "phonemes": Lx}), flush=True)

    # the same work on the host: tests/_prep.py (numpy), best of three
    got = p_out[0].cpu().numpy()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        ph = [P.pitch_target(f0_h[b], dur_h[b])[0] for b in range(B)]
        ex_n, ex_sum = 0, 0.0
        for v in ph:
            kept = v[P.outlier_fence(v)[0]]
            ex_n, ex_sum = ex_n + len(kept), ex_sum + kept.sum()
        P.normalize(ph, np.float64(180.0), np.float64(30.0))
        best = min(best, time.perf_counter() - t0)
    err = max(float(np.abs(got[b] - ph[b]).max()) for b in range(B))
    print(json.dumps({"host_restatement_ms": round(best * 1e3, 2), "max_abs_diff_of_phoneme_means": err}), flush=True)


if __name__ == "__main__":
    main()
