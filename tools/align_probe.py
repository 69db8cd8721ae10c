#!/usr/bin/env python3
"""Time the alignment launches (include/fs2hip_align.h) on a corpus-like batch:

(a) ops.mas, the decision bitmap in LDS and in global memory, against the numpy restatement of
    tests/_align.py on the host;
(b) ForwardSumLoss forward plus backward against torch's own CTC on the same GPU: the usual loop of
    one F.ctc_loss call per utterance, and one batched F.ctc_loss call (both with the log-softmax
    over [blank, logp] that the kernel fuses, and with their backward).

    python tools/align_probe.py [--reps 20] [--rounds 5] [--out profiles/align/headline_runs.txt]

64 utterances x 860 frames x 150 phonemes, float32, full lengths, on device buffers allocated once.
Each round is event-timed over --reps repetitions after a warm-up. One JSON line per round and
mode, one for the host; the lines are also appended to --out. us_per_frame is the time of one step
of the recurrence (one workgroup barrier per frame and utterance; the 64 utterances run side by side).
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
import torch.nn.functional as F  # noqa: E402


def corpus_batch(B=64, T=860, L=150, seed=3):
    """A soft alignment around the diagonal, as a trained aligner emits it: float32 [B, T, L]."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None] / T
    j = (np.arange(L)[None, :] + 0.5) / L
    x = np.empty((B, T, L), dtype=np.float32)
    for b in range(B):
        s = -((t - j) ** 2) * (400.0 + 10.0 * b) + rng.standard_normal((T, L))
        s = s - s.max(axis=1, keepdims=True)
        x[b] = s - np.log(np.exp(s).sum(axis=1, keepdims=True))
    return x


def timed(fn, reps, rounds, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "align", "headline_runs.txt"))
    a = ap.parse_args()
    import fs2amd
    from fs2amd import _lib, ops

    import _align as A

    dev = torch.device("cuda:0")
    x_h = corpus_batch()
    B, T, L = x_h.shape
    x = torch.from_numpy(x_h).to(dev)
    t_lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    l_lens = torch.full((B,), L, dtype=torch.int64, device=dev)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    shape = {"utterances": B, "frames": T, "phonemes": L, "reps": a.reps}
    # (a) the search
    dur = torch.empty(B, L, device=dev, dtype=torch.int64)
    score = torch.empty(B, device=dev, dtype=torch.float64)
    results = {}
    for bm in ("lds", "global"):
        def run(bm=bm):
            ops.mas(x, t_lens, l_lens, bitmap=bm, out=(dur, score, None))
        for rnd, ms in enumerate(timed(run, a.reps, a.rounds, dev)):
            emit(dict(shape, mode=f"mas/{bm}", round=rnd, ms_per_launch=round(ms, 4), us_per_frame=round(1e3 * ms / T, 4),
                      lds_bytes=_lib.mas_lds_bytes(T, L, bm == "lds")))
        results[bm] = (dur.cpu().numpy().copy(), score.cpu().numpy().copy())
    t0 = time.perf_counter()
    n_host = 4
    refs = [A.mas_ref(x_h[b]) for b in range(n_host)]
    dt = time.perf_counter() - t0
    same = all((results[bm][0][b] == refs[b][0]).all() and results[bm][1][b] == refs[b][1]
               for bm in results for b in range(n_host))
    emit({"host_restatement_ms_per_batch_scaled": round(1e3 * dt / n_host * B, 1), "host_utterances_timed": n_host,
          "same_durations_and_score_bits": bool(same),
          "lds_and_global_same": bool((results["lds"][0] == results["global"][0]).all())})

    # (b) the loss, forward plus backward
    crit = fs2amd.ForwardSumLoss()
    xg = x.clone().requires_grad_(True)
    blank = torch.full((B, T, 1), -1.0, device=dev)
    targets = torch.arange(1, L + 1, device=dev)[None].repeat(B, 1)
    in_lens, tg_lens = [T] * B, [L] * B

    def ours():
        xg.grad = None
        crit(xg, t_lens, l_lens).backward()

    def torch_batched():
        xg.grad = None
        lp = F.log_softmax(torch.cat([blank, xg], dim=2), dim=2).transpose(0, 1)
        nll = F.ctc_loss(lp, targets, in_lens, tg_lens, reduction="none", zero_infinity=True)
        (nll / L).mean().backward()

    def torch_loop():
        xg.grad = None
        total = 0.0
        for b in range(B):
            lp = F.log_softmax(torch.cat([blank[b], xg[b]], dim=1), dim=1)[:, None, :]
            total = total + F.ctc_loss(lp, targets[b:b + 1], [T], [L], reduction="sum", zero_infinity=True) / L
        (total / B).backward()

    grads = {}
    for name, fn, reps in (("forward_sum/fwd+bwd", ours, a.reps), ("torch_ctc_batched/fwd+bwd", torch_batched, a.reps),
                           ("torch_ctc_loop/fwd+bwd", torch_loop, max(a.reps // 10, 1))):
        for rnd, ms in enumerate(timed(fn, reps, a.rounds, dev)):
            emit(dict(shape, mode=name, round=rnd, ms_per_call=round(ms, 4), reps=reps,
                      us_per_frame=round(1e3 * ms / (2 * T), 4)))
        grads[name] = xg.grad.double().cpu().numpy().copy()
    ref = grads["torch_ctc_batched/fwd+bwd"]
    emit({"max_abs_grad_diff_vs_torch_batched_f32": float(np.abs(grads["forward_sum/fwd+bwd"] - ref).max()),
          "max_abs_grad_torch_loop_vs_batched": float(np.abs(grads["torch_ctc_loop/fwd+bwd"] - ref).max()),
          "max_abs_grad": float(np.abs(ref).max()), "lds_bytes": _lib.forward_sum_lds_bytes(T, L)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
