#!/usr/bin/env python3
"""Time the two launches of include/fs2hip_resample.h on a corpus-like batch, and
scipy.signal.resample_poly on the host for the same batch.

    python tools/resample_probe.py [--reps 20] [--rounds 5] [--out profiles/resample/headline_runs.txt]

64 utterances of 160,000 int16 samples (10 s) at 16 kHz -> 22,050 Hz (441/320, 8821 taps), on device
buffers allocated once. Each round is event-timed over --reps launches after a warm-up, for
fs2_resample with and without the float64 output, and for fs2_peak_int16. One JSON line per round
and mode, one for the host; the lines are also appended to --out.

Rates. A term is one f64 multiply and one f64 add (never fused), two vector instructions; an output
has hi - lo + 1 of them, 20 or 21 at 441/320. The peak taken is 78.6 TFLOP/s FP64 vector (AMD's
MI355X data sheet: half the 157.3 TFLOP/s FP32 vector figure), i.e. 39.3e12 f64 lane-instructions
per second and 19.65e12 terms per second. The launch also writes 12 (or 4) bytes per output.
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


def corpus_batch(B=64, n=160000, sr=16000.0, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    wav = np.zeros((B, n), dtype=np.int16)
    for b in range(B):
        f = 110.0 + 3.0 * b + 25.0 * np.sin(2 * np.pi * (0.7 + 0.01 * b) * t)
        ph = 2 * np.pi * np.cumsum(f) / sr
        x = sum(np.sin(h * ph) / h for h in range(1, 6)) * (np.sin(2 * np.pi * 1.3 * t + b) > -0.3)
        wav[b] = np.round(6000.0 * x + 40.0 * rng.standard_normal(n)).astype(np.int16)
    return wav


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import ops
    from fs2amd.audio import resample_ratio, resample_taps

    import _resample as R

    dev = torch.device("cuda:0")
    up, down = resample_ratio(22050, 16000)
    wav_h = corpus_batch()
    B, n = wav_h.shape
    M = ops.resample_out_len(n, up, down)
    h0 = resample_taps(up, down)
    _, lo, hi = R.ranges(n, up, down, R.half_len(up, down))
    terms = B * int((hi - lo + 1).sum())
    wav = torch.from_numpy(wav_h).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    taps = torch.from_numpy(h0 * up).to(dev)
    y = torch.empty(B, M, device=dev, dtype=torch.float64)
    y32 = torch.empty(B, M, device=dev, dtype=torch.float32)
    peak = torch.empty(B, device=dev, dtype=torch.float32)
    out_lens = torch.empty(B, device=dev, dtype=torch.int64)
    q = torch.empty(B, M, device=dev, dtype=torch.int16)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(dev)
        for rnd in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            yield rnd, e0.elapsed_time(e1) / a.reps

    for mode, out in (("resample y32+peak", (None, y32, peak, out_lens)), ("resample y+y32+peak", (y, y32, peak, out_lens))):
        for rnd, ms in timed(lambda: ops.resample(wav, lens, up=up, down=down, taps=taps, out=out)):
            nbytes = B * M * (4 if out[0] is None else 12) + wav_h.nbytes
            emit({"mode": mode, "round": rnd, "ms_per_launch": round(ms, 4), "reps": a.reps, "utterances": B,
                  "samples_in": n, "samples_out": M, "terms": terms, "terms_per_s": round(terms / (ms * 1e-3), 1),
                  "fraction_of_f64_vector_peak": round(terms / (ms * 1e-3) / PEAK_TERMS_PER_S, 4),
                  "gbytes_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    for rnd, ms in timed(lambda: ops.peak_int16(y32, peak, out_lens, out=q)):
        emit({"mode": "peak_int16", "round": rnd, "ms_per_launch": round(ms, 4), "reps": a.reps,
              "gbytes_per_s": round(B * M * 6 / (ms * 1e-3) / 1e9, 1)})

    # the host: scipy on the project's taps, two utterances timed and scaled to the batch
    ref = {"host": "scipy.signal.resample_poly", "s_per_batch_scaled": None}
    try:
        from scipy.signal import resample_poly

        t0 = time.perf_counter()
        r = [resample_poly(wav_h[b].astype(np.float64), up, down, window=h0) for b in range(2)]
        ref["s_per_batch_scaled"] = round((time.perf_counter() - t0) / 2 * B, 3)
        ref["first_two_utterances_same_bits"] = bool(
            all((y[b].cpu().numpy().view(np.uint64) == r[b].view(np.uint64)).all() for b in range(2)))
    except ImportError:
        pass
    ref["int16_peak_abs"] = int(q.to(torch.int32).abs().max())
    emit(ref)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
