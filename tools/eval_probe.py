#!/usr/bin/env python3
"""Time the evaluation launches (include/fs2hip_eval.h) on a corpus-like batch:

(a) ops.dtw with the step bitmap in the workspace at 64 utterances x 860 x 860 frames, D = 13, float32
    (the full-length case: no 2-bit layout of 860 x 860 fits the LDS), and in LDS and in the workspace
    at 64 x 512 x 512;
(b) ops.pair_dist at the same sizes: what materialising the cost matrix would cost before the
    programme read a single value of it back (the DTW computes its costs where it uses them);
(c) the numpy restatement of tests/_eval.py on a few utterances on the host, scaled to 64;
(d) ops.mas at 64 x 860 x 150 in the same process, for scale (half as many sequential steps).

    python tools/eval_probe.py [--reps 50] [--rounds 5] [--out profiles/eval/headline_runs.txt]

Full lengths, on device buffers allocated once. Each round is event-timed over --reps repetitions
after a warm-up. One JSON line per round and mode; the lines are also appended to --out.
us_per_diagonal is the time of one step of the recurrence (one workgroup barrier per anti-diagonal and
utterance; the 64 utterances run side by side).
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import _lib, ops

    import _eval as E

    dev = torch.device("cuda:0")
    B, D = 64, 13
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    for T, modes in ((860, ("global",)), (512, ("lds", "global"))):
        x_h = np.stack([E.make_feats(T, D, 2 * b) for b in range(B)]).astype(np.float32)
        y_h = np.stack([E.make_feats(T, D, 2 * b + 1) for b in range(B)]).astype(np.float32)
        x, y = torch.from_numpy(x_h).to(dev), torch.from_numpy(y_h).to(dev)
        lens = torch.full((B,), T, dtype=torch.int64, device=dev)
        P = 2 * T - 1
        out = (torch.empty(B, device=dev, dtype=torch.float64), torch.empty(B, device=dev, dtype=torch.int32),
               torch.empty(B, P, device=dev, dtype=torch.int32), torch.empty(B, P, device=dev, dtype=torch.int32))
        shape = {"utterances": B, "frames_x": T, "frames_y": T, "D": D, "reps": a.reps}
        results = {}
        for bm in modes:
            def run(bm=bm):
                ops.dtw(x, lens, y, lens, bitmap=bm, out=out)
            for rnd, ms in enumerate(timed(run, a.reps, a.rounds, dev)):
                emit(dict(shape, mode=f"dtw/{bm}", round=rnd, ms_per_launch=round(ms, 4),
                          us_per_diagonal=round(1e3 * ms / P, 4), lds_bytes=_lib.dtw_lds_bytes(T, T, bm == "lds"),
                          ws_bytes=_lib.dtw_ws_bytes(B, T, T) if bm == "global" else 0))
            results[bm] = tuple(t.cpu().numpy().copy() for t in out)
        cost = torch.empty(B, T, T, device=dev, dtype=torch.float64)
        for rnd, ms in enumerate(timed(lambda: ops.pair_dist(x, lens, y, lens, out=cost), a.reps, a.rounds, dev)):
            emit(dict(shape, mode="pair_dist", round=rnd, ms_per_launch=round(ms, 4), out_bytes=cost.numel() * 8))
        n_host = 2
        cost_h = cost[:n_host].cpu().numpy()
        t0 = time.perf_counter()
        refs = [E.dtw_ref(x_h[b], y_h[b]) for b in range(n_host)]
        dt = time.perf_counter() - t0
        over = [E.dtw_from_cost(cost_h[b]) for b in range(n_host)]
        same = all(r[0][b] == o[0] and r[1][b] == o[1] and (r[2][b, :o[1]] == o[2]).all() and (r[3][b, :o[1]] == o[3]).all()
                   for r in results.values() for b, o in enumerate(over))
        emit(dict(shape, host_restatement_ms_per_batch_scaled=round(1e3 * dt / n_host * B, 1), host_utterances_timed=n_host,
                  same_bits_as_recursion_over_gpu_costs=bool(same),
                  same_paths_as_pure_host=all((results[modes[0]][2][b, :r[1]] == r[2]).all() for b, r in enumerate(refs)),
                  forms_agree=all(all((u == v).all() for u, v in zip(results[modes[0]], r)) for r in results.values())))

    # (d) the search of include/fs2hip_align.h, for scale
    T, L = 860, 150
    logp = torch.log_softmax(torch.randn(B, T, L, device=dev, generator=torch.Generator(dev).manual_seed(3)), dim=2)
    t_lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    l_lens = torch.full((B,), L, dtype=torch.int64, device=dev)
    mas_out = (torch.empty(B, L, device=dev, dtype=torch.int64), torch.empty(B, device=dev, dtype=torch.float64), None)
    for rnd, ms in enumerate(timed(lambda: ops.mas(logp, t_lens, l_lens, out=mas_out), a.reps, a.rounds, dev)):
        emit({"utterances": B, "frames": T, "phonemes": L, "reps": a.reps, "mode": "mas/auto", "round": rnd,
              "ms_per_launch": round(ms, 4), "us_per_frame": round(1e3 * ms / T, 4)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
