#!/usr/bin/env python3
"""Time the three entry points of include/fs2hip_iir.h on a corpus-like batch, and the same result on the
host (scipy.signal.sosfilt plus numpy gating; torch has no recursive filter to compose one from).

    python tools/loudness_probe.py [--reps 30] [--rounds 5] [--out profiles/loudness/headline_runs.txt]

64 utterances of 220,500 int16 samples (10 s at 22,050 Hz), K-weighting (two sections), a gating hop of
2,205 samples, on device buffers allocated once. Each round is event-timed over --reps calls after a
warm-up: the C entry points themselves through ctypes, so that no torch operation of the wrappers is
inside the window. One JSON line per round and mode; the lines are also appended to --out.

Bytes. fs2_sosfilt has to read every sample once and write every y: B * n * (2 + 8) bytes;
fs2_loudness_gate has to read y once: B * n * 8; fs2_gain_int16 reads and writes every sample, and reads
it once more for the peak when a ceiling is given: B * n * (2 + 2 [+ 2]). Each over the elapsed time is
given as a fraction of 8.0 TB/s (the HBM3E data-sheet peak; a float4 copy reaches about 6.3 TB/s on this
part). fs2_sosfilt is not bound by that traffic: one workgroup per row leaves three compute units in
four idle at B = 64, and inside a workgroup the 64 dependent steps of a block's recurrence (eight float64
operations deep each) are a latency chain that no other wave of the workgroup can hide. --rows 256
shows the same kernel with every compute unit busy.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loudness", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import _lib as L_, loudness, ops
    from vad_probe import corpus_batch

    import _loudness as R

    lib = L_.load()
    dev = torch.device("cuda:0")
    fs = 22050
    wav_h = corpus_batch(B=a.rows)
    B, n = wav_h.shape
    H = R.gate_hop(fs)
    S = 2
    wav = torch.from_numpy(wav_h).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    kw = loudness.KWeighting(fs, dev)
    sos = torch.from_numpy(kw.sos).to(dev)
    y = torch.empty(B, n, device=dev, dtype=torch.float64)
    zbar = torch.empty(B, device=dev, dtype=torch.float64)
    counts = torch.empty(B, 3, device=dev, dtype=torch.int32)
    ws_bytes = int(lib.fs2_loudness_workspace_bytes(B, n, H))
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
    q = torch.empty(B, n, device=dev, dtype=torch.int16)
    gain = torch.empty(B, device=dev, dtype=torch.float64)
    clipped = torch.empty(B, device=dev, dtype=torch.int32)
    unmeasured = torch.empty(B, device=dev, dtype=torch.int32)
    peak = torch.empty(B, device=dev, dtype=torch.float64)
    ptr, stream = ops._ptr, ops._stream(wav)
    ga, tz = R.abs_gate(np.int16), R.target_z(-23.0, np.int16)

    def sosfilt():
        L_.check(lib.fs2_sosfilt(ptr(wav), L_.FS2_I16, n, ptr(lens), B, n, ptr(sos), ptr(kw.tables), S, None, ptr(y), None,
                                 None, stream), "fs2_sosfilt")

    def gate():
        L_.check(lib.fs2_loudness_gate(ptr(y), ptr(lens), B, n, H, ga, 0.1, ptr(zbar), ptr(counts), ptr(ws), ws_bytes,
                                       stream), "fs2_loudness_gate")

    def apply(ceiling=0.0):
        L_.check(lib.fs2_gain_int16(ptr(wav), L_.FS2_I16, n, ptr(lens), B, n, ptr(zbar), tz, ceiling, ptr(q), ptr(gain),
                                    ptr(clipped), ptr(unmeasured), ptr(peak) if ceiling > 0.0 else None, stream),
                 "fs2_gain_int16")

    def whole():
        sosfilt()
        gate()
        apply()

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

    shape = {"utterances": B, "samples": n, "sections": S, "hop": H, "reps": a.reps, "layout": "one workgroup per row"}

    def rate(nbytes, ms):
        return {"bytes": nbytes, "gbytes_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                "fraction_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}

    dev_ms = {}
    for name, fn, nbytes in (("fs2_sosfilt", sosfilt, B * n * 10), ("fs2_loudness_gate", gate, B * n * 8),
                             ("fs2_gain_int16", apply, B * n * 4),
                             ("fs2_gain_int16 with a peak ceiling", lambda: apply(30000.0), B * n * 6),
                             ("sosfilt + gate + gain (normalize_loudness, device part)", whole, B * n * 6)):
        for rnd, ms in timed(fn):
            emit(dict(shape, mode=name, round=rnd, ms_per_call=round(ms, 4), **rate(nbytes, ms)))
            dev_ms[name] = min(ms, dev_ms.get(name, ms))
    whole()
    torch.cuda.synchronize(dev)
    zb_dev, q_dev = zbar.cpu().numpy(), q.cpu().numpy()

    # the host: scipy's sosfilt over the batch, numpy gating and gain, float64
    from scipy import signal

    def host():
        yh = signal.sosfilt(kw.sos, wav_h.astype(np.float64), axis=1)
        J = R.blocks(n, H)
        sq = yh * yh
        cs = np.concatenate([np.zeros((B, 1)), np.cumsum(sq, axis=1)], axis=1)
        z = (cs[:, 4 * H:4 * H + J * H:H] - cs[:, 0:J * H:H]) / (4 * H)
        zb = np.zeros(B)
        for b in range(B):
            A = z[b] > ga
            if A.any():
                Rm = A & (z[b] > 0.1 * z[b][A].mean())
                zb[b] = z[b][Rm].mean() if Rm.any() else 0.0
        g = np.where(zb > 0, np.sqrt(tz / np.where(zb > 0, zb, 1.0)), 1.0)
        return zb, np.clip(np.rint(wav_h * g[:, None]), -32768, 32767).astype(np.int16)

    host()
    best = None
    for rnd in range(3):
        t0 = time.perf_counter()
        zb_h, q_h = host()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
        emit(dict(shape, mode="host: scipy.signal.sosfilt + numpy gating and gain (float64)", round=rnd,
                  ms_per_call=round(ms, 2)))
    lu = np.abs(10 * np.log10(zb_dev / zb_h))
    emit({"check": "device against host: loudness difference in LU, samples that differ by more than one count",
          "max_lu_difference": float(lu.max()), "samples_off_by_more_than_1": int((np.abs(q_dev.astype(np.int32) - q_h) > 1).sum()),
          "samples_that_differ": int((q_dev != q_h).sum()),
          "host_over_device": round(best / dev_ms["sosfilt + gate + gain (normalize_loudness, device part)"], 1)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
