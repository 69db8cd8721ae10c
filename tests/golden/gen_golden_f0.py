#!/usr/bin/env python3
"""Generate tests/golden/f0_a.npz: synthetic waveforms, the contours the numpy restatement of
include/fs2hip_f0.h (tests/_f0.py) gives for them, and the true F0 where one is defined.

Deterministic (numpy's default_rng with fixed seeds); needs nothing but numpy. The reference's own
estimator (pyworld) is not involved: see tests/_f0.py.

    wav16 / lens16 / names16   int16 cases at sr 22050, hop 256, W 1024, with f0_16 / tau_16
                               [N, F_max] (0 past the utterance) and truth16 (Hz; NaN = undefined)
    wav200 / lens200 ...       int16 cases at hop 200, W 800
    wav32 / lens32 ...         float32: row 0 = wav16[twin16] / 32768, row 1 = a float64 mixture
                               rounded to float32 (not dyadic)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_f0.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _f0 as Y  # noqa: E402

SR = Y.SR
AMP = 7000.0


def tone(f, n, harmonics=range(1, 6), phase=0.3):
    t = np.arange(n) / SR
    return sum(np.sin(2 * np.pi * f * h * t + phase * h) / h for h in harmonics)


def glide(n, f_a=120.0, rate=200.0):
    t = np.arange(n) / SR
    ph = 2 * np.pi * (f_a * t + 0.5 * rate * t * t)
    return sum(np.sin(h * ph) / h for h in range(1, 6)), f_a + rate * t


def i16(x):
    return np.round(AMP * np.asarray(x)).astype(np.int16)


def frame_truth(n, hop, value):
    """value (a number, or a per-sample track) at the frame centres k * hop."""
    F = Y.n_frames(n, hop)
    if np.ndim(value) == 0:
        return np.full(F, float(value))
    return np.asarray(value)[np.minimum(np.arange(F) * hop, max(n - 1, 0))] if n else np.full(F, np.nan)


def splice(rng, parts):
    """parts: (kind, n, f) with kind 's' silence, 't' tone, 'n' noise -> (waveform, per-sample truth)."""
    xs, tr = [], []
    for kind, n, f in parts:
        xs.append(np.zeros(n) if kind == "s" else tone(f, n) if kind == "t" else 0.5 * rng.standard_normal(n))
        tr.append(np.full(n, np.nan))  # voicing switches inside frames: no truth claimed
    return np.concatenate(xs), np.concatenate(tr)


def pack(arrays, dtype):
    lens = np.array([len(a) for a in arrays], dtype=np.int64)
    out = np.zeros((len(arrays), max(int(lens.max()), 1)), dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out, lens


def contours(wavs, hop, W):
    f0s, taus = [], []
    for w in wavs:
        f0, tau, _ = Y.contour(w, hop=hop, W=W)
        f0s.append(f0)
        taus.append(tau)
    return pack(f0s, np.float64)[0], pack(taus, np.int32)[0]


def main():
    rng = np.random.default_rng(20240607)
    cases = []  # (name, int16 waveform, truth per frame)

    def add(name, x, truth, hop=Y.HOP):
        x = i16(x)
        cases.append((name, x, frame_truth(len(x), hop, truth)))

    add("silence_0", np.zeros(0), np.nan)
    for n in (1, 255, 256, 257, 512, 1334, 1335, 1336):  # 1334..1336 straddle W + tau_max
        add(f"tone220_{n}", tone(220.0, n), 220.0)
    for f in (75.0, 100.0, 163.7, 440.0, 780.0):
        add(f"tone{f:g}", tone(f, 3001), f)
    add("tone220", tone(220.0, 9001), 220.0)  # more than one frame group and a ragged tail
    add("tone71.5", tone(71.5, 3100), 71.5)
    add("tone71.1", tone(71.1, 3100), 71.1)  # the lag lands at tau_max - 1
    add("tone860", tone(860.0, 3000), np.nan)  # above the range: 0, or the sub-octave
    g, g_f = glide(8821)
    add("glide120_200", g, g_f)
    add("missing_fundamental", tone(150.0, 3000, harmonics=range(2, 7)) + 0.01 * rng.standard_normal(3000), 150.0)
    add("noise", 0.5 * rng.standard_normal(3000), np.nan)
    add("silence", np.zeros(3000), np.nan)
    add("splice_a", *splice(rng, [("s", 700, 0), ("t", 2900, 130.0), ("n", 2500, 0), ("t", 2933, 310.0)]))
    add("splice_b", *splice(rng, [("t", 1500, 95.0), ("s", 1111, 0), ("n", 900, 0), ("t", 2600, 523.0)]))
    names = [c[0] for c in cases]
    wav16, lens16 = pack([c[1] for c in cases], np.int16)
    f0_16, tau_16 = contours([c[1] for c in cases], Y.HOP, Y.WIN)
    truth16 = np.full(f0_16.shape, np.nan)
    for b, c in enumerate(cases):
        truth16[b, :len(c[2])] = c[2]

    c200 = [i16(tone(220.0, 3003)), i16(splice(rng, [("s", 450, 0), ("t", 2000, 180.0), ("n", 777, 0)])[0]),
            i16(tone(100.0, 199)), i16(tone(100.0, 200))]
    wav200, lens200 = pack(c200, np.int16)
    f0_200, tau_200 = contours(c200, 200, 800)

    twin = names.index("tone163.7")
    mix = 0.31 * tone(187.3, 4000) + 0.11 * tone(411.0, 4000, harmonics=(1, 2)) + 0.003 * rng.standard_normal(4000)
    c32 = [(cases[twin][1].astype(np.float64) / 32768.0).astype(np.float32), mix.astype(np.float32)]
    dp_general = Y.table(c32[1])[1]
    bad = Y.fragile(dp_general)
    if bad:
        raise SystemExit(f"the general float32 case has fragile frames, redraw it: {bad[:5]}")
    wav32, lens32 = pack(c32, np.float32)
    f0_32, tau_32 = contours(c32, Y.HOP, Y.WIN)

    out = os.path.join(HERE, "f0_a.npz")
    np.savez_compressed(out, wav16=wav16, lens16=lens16, names16=np.array(names), f0_16=f0_16, tau_16=tau_16,
                        truth16=truth16, wav200=wav200, lens200=lens200, f0_200=f0_200, tau_200=tau_200,
                        wav32=wav32, lens32=lens32, f0_32=f0_32, tau_32=tau_32, twin16=np.int64(twin))
    print(out, os.path.getsize(out), "bytes")
    for b, n in enumerate(names):
        F = Y.n_frames(int(lens16[b]), Y.HOP)
        print(f"{n:22s} n {int(lens16[b]):5d} voiced {int((f0_16[b, :F] > 0).sum()):3d}/{F:3d} "
              f"tau {tau_16[b, :F].min()}..{tau_16[b, :F].max()}")


if __name__ == "__main__":
    main()
