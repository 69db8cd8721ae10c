#!/usr/bin/env python3
"""Time the F0 launch (include/fs2hip_f0.h) on a corpus-like batch, with and without the cmnd table,
and the numpy restatement of tests/_f0.py on the host for scale.

    python tools/f0_probe.py [--reps 20] [--rounds 5] [--out profiles/f0/headline_runs.txt]

64 utterances of 220,000 int16 samples (860 frames each at hop 256), W 1024, lags 27..311, on
device buffers allocated once. Each round is event-timed over --reps launches after a warm-up. One
JSON line per round and mode, one for the host; the lines are also appended to --out.

Rates. The contract's term count is B * F * W * tau_max; the kernel shares the sums of hop-sized
blocks between the W / hop frames over them and pads the lags to a multiple of 8, so it executes
groups * (8 + W / hop - 1) * hop * tau_pad terms: both are reported. A term is one f64 subtract and
one f64 FMA, two vector instructions; the peak taken is 78.6 TFLOP/s FP64 vector (AMD's MI355X data
sheet: half the 157.3 TFLOP/s FP32 vector figure), i.e. 39.3e12 f64 lane-instructions per second
and 19.65e12 executed terms per second.
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

PEAK_TERMS_PER_S = 78.6e12 / 2 / 2


def corpus_batch(B=64, n=220000, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    wav = np.zeros((B, n), dtype=np.int16)
    for b in range(B):
        f = 110.0 + 3.0 * b + 25.0 * np.sin(2 * np.pi * (0.7 + 0.01 * b) * t)
        ph = 2 * np.pi * np.cumsum(f) / 22050.0
        x = sum(np.sin(h * ph) / h for h in range(1, 6)) * (np.sin(2 * np.pi * 1.3 * t + b) > -0.3)
        wav[b] = np.round(6000.0 * x + 40.0 * rng.standard_normal(n)).astype(np.int16)
    return wav


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f0", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import _lib, ops

    import _f0 as Y

    dev = torch.device("cuda:0")
    hop, W = 256, 1024
    tau_min, tau_max = ops.f0_lags(22050, 71.0, 800.0)
    wav_h = corpus_batch()
    B, n = wav_h.shape
    F = n // hop + 1
    wav = torch.from_numpy(wav_h).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    f0 = torch.empty(B, F, device=dev, dtype=torch.float64)
    tau = torch.empty(B, F, device=dev, dtype=torch.int32)
    cmnd = torch.empty(B, F, tau_max + 1, device=dev, dtype=torch.float64)
    kw = dict(sampling_rate=22050, hop_length=hop, win_length=W)
    groups = B * -(-F // _lib.F0_GROUP)
    tau_pad = -(-tau_max // 8) * 8
    nominal = B * F * W * tau_max
    executed = groups * (_lib.F0_GROUP + W // hop - 1) * hop * tau_pad  # the last group of an utterance does less
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    for mode, out in (("f0+tau", (f0, tau, None)), ("f0+tau+cmnd", (f0, tau, cmnd))):
        for _ in range(5):
            ops.f0_yin(wav, lens, out=out, **kw)
        torch.cuda.synchronize(dev)
        for rnd in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                ops.f0_yin(wav, lens, out=out, **kw)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            emit({"mode": mode, "round": rnd, "ms_per_launch": round(ms, 4), "reps": a.reps, "utterances": B,
                  "frames": F, "nominal_terms": nominal, "nominal_terms_per_s": round(nominal / (ms * 1e-3), 1),
                  "executed_terms_upper": executed, "executed_terms_per_s": round(executed / (ms * 1e-3), 1),
                  "fraction_of_f64_vector_peak": round(executed / (ms * 1e-3) / PEAK_TERMS_PER_S, 4)})

    # the restatement on the host: one tenth of one utterance, scaled to the batch by its frame count
    x = wav_h[0, :22016]
    t0 = time.perf_counter()
    r_f0, r_tau, _ = Y.contour(x)
    dt = time.perf_counter() - t0
    same = bool((f0[0, :40].cpu().numpy().view(np.uint64) == r_f0[:40].view(np.uint64)).all())
    emit({"host_restatement_s_per_batch_scaled": round(dt / len(r_f0) * B * F, 1), "host_frames_timed": len(r_f0),
          "first_40_frames_same_bits": same, "voiced_fraction_gpu": round(float((f0 > 0).double().mean()), 3)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
