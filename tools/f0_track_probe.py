#!/usr/bin/env python3
"""Time the F0 tracker (include/fs2hip_f0_track.h) on the corpus-like batch of tools/f0_probe.py: the
tracker alone over a table computed once, the YIN launch with its cmnd table followed by the
tracker, the YIN launch alone (with and without cmnd) in the same session, and the numpy
restatement of tests/_f0_track.py on the host for scale.

    python tools/f0_track_probe.py [--reps 20] [--rounds 5] [--out profiles/f0_track/headline_runs.txt]

64 utterances of 220,000 int16 samples (860 frames each at hop 256), W 1024, lags 27..311, 210 pitch
bins, steps of 12, on device buffers allocated once. Each round is event-timed over --reps launches
after a warm-up. One JSON line per round and mode, one for the host; the lines are also appended to
--out.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def f0_probe():
    spec = importlib.util.spec_from_file_location("f0_probe", os.path.join(REPO, "tools", "f0_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f0_track", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import _lib, ops

    import _f0 as Y
    import _f0_track as T

    dev = torch.device("cuda:0")
    hop, W = 256, 1024
    tau_min, tau_max = ops.f0_lags(22050, 71.0, 800.0)
    wav_h = f0_probe().corpus_batch()
    B, n = wav_h.shape
    F = n // hop + 1
    wav = torch.from_numpy(wav_h).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    f0 = torch.empty(B, F, device=dev, dtype=torch.float64)
    tau = torch.empty(B, F, device=dev, dtype=torch.int32)
    cmnd = torch.empty(B, F, tau_max + 1, device=dev, dtype=torch.float64)
    tf0 = torch.empty(B, F, device=dev, dtype=torch.float64)
    state = torch.empty(B, F, device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float64)
    ws_bytes = _lib.f0_track_workspace_bytes(B, F, tau_min, tau_max, 210)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    ykw = dict(sampling_rate=22050, hop_length=hop, win_length=W)
    tkw = dict(sampling_rate=22050, hop_length=hop, out=(tf0, state, score), workspace=ws)

    def yin():
        ops.f0_yin(wav, lens, out=(f0, tau, None), **ykw)

    def yin_cmnd():
        ops.f0_yin(wav, lens, out=(f0, tau, cmnd), **ykw)

    def track():
        ops.f0_track(cmnd, lens, **tkw)

    def both():
        yin_cmnd()
        track()

    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    yin_cmnd()
    for mode, fn in (("f0_yin", yin), ("f0_yin+cmnd", yin_cmnd), ("f0_track", track), ("f0_yin+cmnd, f0_track", both)):
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
            emit({"mode": mode, "round": rnd, "ms_per_call": round(e0.elapsed_time(e1) / a.reps, 4), "reps": a.reps,
                  "utterances": B, "frames": F, "workspace_bytes": ws_bytes})

    # the restatement on the host: 40 frames of one utterance, scaled to the batch by its frame count
    F_host = 40
    dp = cmnd[0, :F_host].cpu().numpy()
    tb = T.tables()
    t0 = time.perf_counter()
    r_f0, r_state, r_score, _, _, _ = T.track_table(dp, tb)
    dt = time.perf_counter() - t0
    g = ops.f0_track(cmnd[:1, :F_host].contiguous(), torch.tensor([(F_host - 1) * hop]), sampling_rate=22050, hop_length=hop)
    same = bool((g.f0[0].cpu().numpy().view(np.uint64) == r_f0.view(np.uint64)).all()
                and (g.state[0].cpu().numpy() == r_state).all() and g.score[0].item() == r_score)
    plain = Y.contour_of_table(dp)[0]
    emit({"host_restatement_s_per_batch_scaled": round(dt / F_host * B * F, 1), "host_frames_timed": F_host,
          "same_bits_as_gpu": same, "voiced_fraction_track": round(float((tf0 > 0).double().mean()), 3),
          "voiced_fraction_yin": round(float((f0 > 0).double().mean()), 3),
          "host_frames_where_yin_and_track_differ": int((plain != r_f0).sum())})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
