#!/usr/bin/env python3
"""Generate tests/golden/resample_a.npz: synthetic int16 / float32 waveforms and what
scipy.signal.resample_poly gives for them on the project's own taps (tests/_resample.py: taps),
for the six ratios of tests/_resample.py: RATIOS.

Deterministic (numpy's default_rng with a fixed seed); needs numpy and scipy. Nothing is written
unless the numpy restatement of include/fs2hip_resample.h (tests/_resample.py: resample) equals
scipy's output bit for bit on every case.

    per ratio "<up>_<down>":  names_, wav_ (int16 [B, n_max], zero-padded), lens_, y_ (float64
                              [B, M_max], scipy's output, zero-padded)
    wav32 / lens32 / y32_*    float32 at 441/320: row 0 = the int16 case TWIN / 32768 (its output is
                              not stored: it is 2^-15 times the twin's), row 1 = a float64 mixture
                              rounded to float32, with scipy's output y_general

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_resample.py
"""
import os
import sys

import numpy as np
from scipy.signal import resample_poly

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _resample as R  # noqa: E402

AMP = 9000.0
TWIN = "tone_noise"


def tone(f, n, sr):
    t = np.arange(n) / sr
    return sum(np.sin(2 * np.pi * f * h * t + 0.3 * h) / h for h in range(1, 5))


def i16(x):
    return np.round(AMP * np.asarray(x)).astype(np.int16)


def impulse(n, at, value):
    x = np.zeros(n, dtype=np.int16)
    x[at] = value
    return x


def int16_cases(rng, up, down, long_case):
    sr = R.TARGET * down / up
    cases = [("empty", np.zeros(0, dtype=np.int16)),
             ("one", np.array([-32768], dtype=np.int16)),
             ("two", np.array([32767, -12345], dtype=np.int16)),
             (f"impulse_first_{down - 1}", impulse(down - 1, 0, 20000)) if down > 1 else ("three", i16([0.5, -1, 1])),
             (f"impulse_last_{down}", impulse(down, down - 1, -20000)),
             (f"noise_{down + 1}", i16(0.5 * rng.standard_normal(down + 1))),
             ("silence", np.zeros(500, dtype=np.int16)),
             (TWIN, i16(0.6 * tone(180.0, 3001, sr) + 0.1 * rng.standard_normal(3001)))]
    if long_case:
        cases.append(("tone_long", i16(tone(261.6, 9001, sr))))
    return cases


def checked(x, up, down, h0):
    """scipy's output on the project's taps, after checking that the restatement equals it."""
    ref = resample_poly(np.asarray(x).astype(np.float64), up, down, window=h0)
    own = R.resample(x, up, down, h0 * up)
    if ref.shape != own.shape or ref.dtype != np.float64 or not (ref.view(np.uint64) == own.view(np.uint64)).all():
        raise SystemExit(f"the restatement is not scipy's resample_poly at {up}/{down}, n {len(x)}: nothing written")
    return ref


def main():
    rng = np.random.default_rng(20240911)
    out = {}
    for up, down in R.RATIOS:
        h0 = R.taps(up, down)
        cases = int16_cases(rng, up, down, long_case=(up, down) == (441, 320))
        k = R.key(up, down)
        out["names_" + k] = np.array([c[0] for c in cases])
        out["wav_" + k], out["lens_" + k] = R.pack([c[1] for c in cases], np.int16)
        out["y_" + k] = R.pack([checked(c[1], up, down, h0) for c in cases], np.float64)[0]
        print(k, "cases", len(cases), "M_max", out["y_" + k].shape[1])

    up, down = 441, 320
    h0 = R.taps(up, down)
    k = R.key(up, down)
    twin = list(out["names_" + k]).index(TWIN)
    w16 = out["wav_" + k][twin, :out["lens_" + k][twin]]
    sr = R.TARGET * down / up
    mix = 0.31 * tone(187.3, 2500, sr) + 0.11 * tone(411.0, 2500, sr) + 0.003 * rng.standard_normal(2500)
    c32 = [(w16.astype(np.float64) / 32768.0).astype(np.float32), mix.astype(np.float32)]
    y_twin = checked(c32[0], up, down, h0)
    if not (y_twin * 32768.0 == out["y_" + k][twin, :len(y_twin)]).all():
        raise SystemExit("the float32 twin is not 2^-15 times its int16 case")
    out["wav32"], out["lens32"] = R.pack(c32, np.float32)
    out["y_general"] = checked(c32[1], up, down, h0)
    out["twin"] = np.int64(twin)

    path = os.path.join(HERE, "resample_a.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
