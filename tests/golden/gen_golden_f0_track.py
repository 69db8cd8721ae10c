#!/usr/bin/env python3
"""Generate tests/golden/f0_track_a.npz: synthetic waveforms, the paths the numpy restatement of
include/fs2hip_f0_track.h (tests/_f0_track.py) gives for them, and the true F0 where one is defined.

Deterministic (numpy's default_rng with fixed seeds); needs nothing but numpy. No estimator of the
reference's is involved: see tests/_f0_track.py.

    wav16 / lens16 / names16   int16 cases at sr 22050, hop 256, W 1024, with f0_16 / state_16
                               [N, F_max] (0 / -1 past the utterance), score_16 [N] and truth16
                               (Hz; NaN = undefined)
    wav200 / lens200 ...       int16 cases at hop 200, W 800
    wav32 / lens32 ...         float32: row 0 = wav16[twin16] / 32768, row 1 = a float64 mixture
                               rounded to float32 (not dyadic)

The conditions tests/test_f0_track_host.py asserts are checked here first (T.fixture_faults): a
fixture that misses one is not written.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_f0_track.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _f0 as Y  # noqa: E402
import _f0_track as T  # noqa: E402
from gen_golden_f0 import frame_truth, glide, i16, pack, splice, tone  # noqa: E402

SR = Y.SR


def tracks(wavs, tb, hop, W):
    f0s, sts, scores = [], [], []
    for w in wavs:
        f0, st, score, _, _, _ = T.track(w, tb, hop, W)
        f0s.append(f0)
        sts.append(st)
        scores.append(score)
    F = max(len(f) for f in f0s)
    f0 = np.zeros((len(wavs), F))
    st = np.full((len(wavs), F), -1, dtype=np.int32)
    for b in range(len(wavs)):
        f0[b, :len(f0s[b])], st[b, :len(sts[b])] = f0s[b], sts[b]
    return f0, st, np.array(scores, dtype=np.float64)


def main():
    rng = np.random.default_rng(20240819)
    tb = T.tables()
    cases = []  # (name, int16 waveform, truth per frame)

    def add(name, x, truth):
        x = i16(x)
        cases.append((name, x, frame_truth(len(x), Y.HOP, truth)))

    n = 9001
    t = np.arange(n) / SR
    add("silence_0", np.zeros(0), np.nan)
    for m in (1, 255, 256, 257, 1335):  # 1335 = W + tau_max
        add(f"tone220_{m}", tone(220.0, m), 220.0)
    add("tone860", tone(860.0, 3000), np.nan)  # above the range
    add("noise", 0.5 * rng.standard_normal(3000), np.nan)
    add("silence", np.zeros(3000), np.nan)
    for f in (75.0, 100.0, 163.7, 220.0, 440.0, 780.0):
        add(f"tone{f:g}", tone(f, n), f)
    g, g_f = glide(8821)
    add("glide120_200", g, g_f)
    add("missing_fundamental", tone(150.0, 9000, harmonics=range(2, 7)) + 0.01 * rng.standard_normal(9000), 150.0)
    add("splice", *splice(rng, [("t", 2900, 130.0), ("n", 2800, 0), ("t", 3300, 310.0)]))
    # the octave trap: a burst of the second subharmonic lifts the trough at the period above plain
    # YIN's threshold for a few frames, and the trough at twice the period is the first below it
    env = np.exp(-0.5 * ((t - 0.2) / 0.03) ** 2)
    add("trap", tone(200.0, n) + 0.5 * env * tone(100.0, n, harmonics=(1, 3)), 200.0)
    # the weak trough: noise holds the trough at the period around plain YIN's threshold
    add("weak", tone(180.0, n) + 0.29 * rng.standard_normal(n), 180.0)
    names = [c[0] for c in cases]
    wav16, lens16 = pack([c[1] for c in cases], np.int16)
    f0_16, state_16, score_16 = tracks([c[1] for c in cases], tb, Y.HOP, Y.WIN)
    truth16 = np.full(f0_16.shape, np.nan)
    for b, c in enumerate(cases):
        truth16[b, :len(c[2])] = c[2]

    c200 = [i16(tone(220.0, 3003)), i16(splice(rng, [("s", 450, 0), ("t", 2000, 180.0), ("n", 777, 0)])[0])]
    wav200, lens200 = pack(c200, np.int16)
    f0_200, state_200, score_200 = tracks(c200, tb, 200, 800)

    twin = names.index("tone163.7")
    mix = 0.31 * tone(187.3, 4000) + 0.11 * tone(411.0, 4000, harmonics=(1, 2)) + 0.003 * rng.standard_normal(4000)
    c32 = [(cases[twin][1].astype(np.float64) / 32768.0).astype(np.float32), mix.astype(np.float32)]
    wav32, lens32 = pack(c32, np.float32)
    f0_32, state_32, score_32 = tracks(c32, tb, Y.HOP, Y.WIN)

    z = dict(wav16=wav16, lens16=lens16, names16=np.array(names), f0_16=f0_16, state_16=state_16, score_16=score_16,
             truth16=truth16, wav200=wav200, lens200=lens200, f0_200=f0_200, state_200=state_200, score_200=score_200,
             wav32=wav32, lens32=lens32, f0_32=f0_32, state_32=state_32, score_32=score_32, twin16=np.int64(twin))
    faults = T.fixture_faults(z, verbose=True)
    if faults:
        raise SystemExit("the fixture misses its conditions, not written:\n  " + "\n  ".join(faults))
    out = os.path.join(HERE, "f0_track_a.npz")
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")
    for b, name in enumerate(names):
        F = Y.n_frames(int(lens16[b]), Y.HOP)
        print(f"{name:22s} n {int(lens16[b]):5d} voiced {int((f0_16[b, :F] > 0).sum()):3d}/{F:3d} score {score_16[b]:.3f}")


if __name__ == "__main__":
    main()
