#!/usr/bin/env python3
"""Time the three entry points of include/fs2hip_vad.h on a corpus-like batch, and a torch composition
of the same result on the same GPU.

    python tools/vad_probe.py [--reps 50] [--rounds 5] [--out profiles/vad/headline_runs.txt]

64 utterances of 220,500 int16 samples (10 s at 22,050 Hz), frame_length 1024, hop 256, top_db 60, on
device buffers allocated once. Each round is event-timed over --reps calls after a warm-up: the C entry
points themselves through ctypes (fs2_vad_power is two launches, its tile sums and the row maximum),
so that no torch operation of the wrappers is inside the window. One JSON line per round and mode; the
lines are also appended to --out.

The yardstick is torch on the same device: unfold over the zero-padded float64 batch, square, mean,
amax, compare, first / last active index (the trim alone: torch has no interval table to offer). It is
timed the same way, in float64 (what the contract computes in) and in float32 (what a user in a hurry
would write; other bits).

Bytes. fs2_vad_power has to read every sample once and write every P: B * n * 2 + B * F * 8 bytes; that
over the elapsed time is given as a fraction of 8.0 TB/s (the HBM3E data-sheet peak; a float4 copy
reaches about 6.3 TB/s on this part). The same ratio for the cut: read and written rows.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def corpus_batch(B=64, n=220500, sr=22050.0, seed=3):
    """Harmonic tones gated into phrases, a noise bed 45 dB down, 0.1 - 0.5 s of near silence at both ends."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    wav = np.zeros((B, n), dtype=np.int16)
    for b in range(B):
        f = 110.0 + 3.0 * b + 25.0 * np.sin(2 * np.pi * (0.7 + 0.01 * b) * t)
        ph = 2 * np.pi * np.cumsum(f) / sr
        x = sum(np.sin(h * ph) / h for h in range(1, 6)) * (np.sin(2 * np.pi * 1.3 * t + b) > -0.3)
        lead, tail = int(sr * (0.1 + 0.4 * rng.random())), int(sr * (0.1 + 0.4 * rng.random()))
        x[:lead] = 0.0
        x[n - tail:] = 0.0
        wav[b] = np.round(6000.0 * x + 2.0 * rng.standard_normal(n)).astype(np.int16)
    return wav


def torch_trim(wav, L, hop, threshold, floor, dtype):
    """(start, end) per row by the header's rule, composed of torch operations."""
    x = torch.nn.functional.pad(wav.to(dtype), (L // 2, L - L // 2))
    P = x.unfold(1, L, hop)[:, :1 + wav.shape[1] // hop].square().mean(dim=2)
    ref = P.amax(dim=1, keepdim=True).clamp(min=floor)
    act = P.clamp(min=floor) > threshold * ref
    F = act.shape[1]
    idx = torch.arange(F, device=wav.device)
    first = torch.where(act, idx, F).amin(dim=1)
    last = torch.where(act, idx, -1).amax(dim=1)
    any_ = last >= 0
    start = torch.where(any_, first * hop, 0)
    end = torch.where(any_, ((last + 1) * hop).clamp(max=wav.shape[1]), 0)
    return P, torch.stack([start, end], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vad", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import _lib as L_, ops

    import _vad as V

    lib = L_.load()
    dev = torch.device("cuda:0")
    L, hop = 1024, 256
    thr, floor = V.threshold_of(60.0), V.floor_of(np.int16)
    wav_h = corpus_batch()
    B, n = wav_h.shape
    F = V.frames(n, hop)
    cap = (F + 1) // 2
    wav = torch.from_numpy(wav_h).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    P = torch.empty(B, F, device=dev, dtype=torch.float64)
    Pmax = torch.empty(B, device=dev, dtype=torch.float64)
    ws_bytes = int(lib.fs2_vad_workspace_bytes(B, F, L, hop))
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
    active = torch.empty(B, F, device=dev, dtype=torch.uint8)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    iv = torch.empty(B, cap, 2, device=dev, dtype=torch.int64)
    trim = torch.empty(B, 2, device=dev, dtype=torch.int64)
    ptr, stream = ops._ptr, ops._stream(wav)

    def power():
        L_.check(lib.fs2_vad_power(ptr(wav), L_.FS2_I16, n, ptr(lens), B, n, L, hop, ptr(P), ptr(Pmax), ptr(ws), ws_bytes,
                                   stream), "fs2_vad_power")

    def intervals():
        L_.check(lib.fs2_vad_intervals(ptr(P), ptr(Pmax), ptr(lens), B, n, hop, thr, floor, 1, 0, cap, 0, ptr(active),
                                       ptr(count), ptr(iv), ptr(trim), stream), "fs2_vad_intervals")

    power()
    intervals()
    trim_h = trim.cpu().numpy()
    M = int((trim_h[:, 1] - trim_h[:, 0]).max())
    rows = torch.empty(B, M, device=dev, dtype=torch.int16)
    out_lens = torch.empty(B, device=dev, dtype=torch.int64)

    def cut():
        L_.check(lib.fs2_vad_cut(ptr(wav), L_.FS2_I16, n, ptr(trim), B, n, M, ptr(rows), ptr(out_lens), stream),
                 "fs2_vad_cut")

    def all_three():
        power()
        intervals()
        cut()

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

    shape = {"utterances": B, "samples": n, "frames": F, "frame_length": L, "hop": hop, "reps": a.reps}
    pbytes = wav_h.nbytes + B * F * 8
    for rnd, ms in timed(power):
        emit(dict(shape, mode="fs2_vad_power", round=rnd, ms_per_call=round(ms, 4), bytes=pbytes,
                  gbytes_per_s=round(pbytes / (ms * 1e-3) / 1e9, 1),
                  fraction_of_hbm_peak=round(pbytes / (ms * 1e-3) / HBM_PEAK, 4)))
    for rnd, ms in timed(intervals):
        emit(dict(shape, mode="fs2_vad_intervals", round=rnd, ms_per_call=round(ms, 4), max_intervals=cap))
    cbytes = int((trim_h[:, 1] - trim_h[:, 0]).sum()) * 2 + B * M * 2
    for rnd, ms in timed(cut):
        emit(dict(shape, mode="fs2_vad_cut", round=rnd, ms_per_call=round(ms, 4), M_max=M, bytes=cbytes,
                  fraction_of_hbm_peak=round(cbytes / (ms * 1e-3) / HBM_PEAK, 4)))
    for rnd, ms in timed(all_three):
        emit(dict(shape, mode="power + intervals + cut", round=rnd, ms_per_call=round(ms, 4)))
    for dt in (torch.float64, torch.float32):
        f = floor if dt == torch.float64 else float(np.float32(floor))
        for rnd, ms in timed(lambda: torch_trim(wav, L, hop, thr, f, dt)):
            emit(dict(shape, mode=f"torch composition {str(dt).split('.')[-1]} (power, mask, trim; no intervals, no cut)",
                      round=rnd, ms_per_call=round(ms, 4)))
    Pt, tt = torch_trim(wav, L, hop, thr, floor, torch.float64)
    emit({"check": "int16 input: every sum is exact, so torch's float64 power and trim must equal the kernels'",
          "power_equal": bool((Pt == P).all()), "trim_equal": bool((tt == trim).all()),
          "mean_trimmed_fraction": round(1.0 - float((trim_h[:, 1] - trim_h[:, 0]).mean()) / n, 4),
          "mean_intervals": round(float(count.float().mean()), 2)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
