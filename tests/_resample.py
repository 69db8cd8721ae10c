"""The resampler and the int16 rule of include/fs2hip_resample.h restated in plain numpy, operation
for operation: the oracle of the resampling tests beside scipy.signal.resample_poly itself, which
the restatement equals bit for bit (tests/golden/gen_golden_resample.py refuses to write the fixture
otherwise; tests/test_resample_host.py checks it again where scipy is installed).

``resample`` walks the tap step: step j adds, for every output at once, the term of its (lo + j)-th
input sample, so each output's sum keeps the header's order (ascending input index) while the loop
runs ceil(N / up) times, not once per output. numpy has no fused multiply-add: the product is
rounded, then added, as the header demands.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TARGET = 22050
RATIOS = ((441, 320), (147, 320), (1, 2), (441, 160), (147, 160), (320, 441))
# 16000, 48000, 44100, 8000 and 24000 Hz -> 22050 Hz, and one ratio with down > up > 1
MAX_WAV_VALUE = 32768.0


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "resample_a.npz")))


def key(up, down):
    return f"{up}_{down}"


def ratio(target, source):
    g = math.gcd(int(target), int(source))
    return int(target) // g, int(source) // g


def half_len(up, down):
    return 10 * max(up, down)


def out_len(n, up, down):
    """ceil(n * up / down) in Python integers."""
    return -(-n * up // down) if n > 0 else 0


def taps(up, down, beta=5.0):
    """The header's design h0 (what fs2amd.audio.resample_taps returns), restated."""
    half = half_len(up, down)
    c = 1.0 / max(up, down)
    h = c * np.sinc(c * (np.arange(2 * half + 1, dtype=np.float64) - half)) * np.kaiser(2 * half + 1, beta)
    return h / h.sum()


def ranges(n, up, down, half):
    """(c, lo, hi) int64 [M] of the header for an utterance of n samples."""
    m = np.arange(out_len(n, up, down), dtype=np.int64)
    c = m * down + half
    lo = np.maximum(0, -((2 * half - c) // up))  # ceil((c - 2 half) / up)
    hi = np.minimum(n - 1, c // up)
    return c, lo, hi


def resample(x, up, down, h):
    """y float64 [ceil(n up / down)] of samples x (int16 or float32) with the kernel's taps
    h = h0 * up."""
    x = np.asarray(x).astype(np.float64)
    n = len(x)
    if up == 1 and down == 1:
        return x.copy()
    h = np.asarray(h, dtype=np.float64)
    half = (len(h) - 1) // 2
    assert len(h) == 2 * half + 1 and half == half_len(up, down)
    c, lo, hi = ranges(n, up, down, half)
    y = np.zeros(len(c))
    for j in range(int((hi - lo + 1).max(initial=0))):
        i = lo + j
        ok = i <= hi
        i = np.where(ok, i, 0)
        k = np.where(ok, c - i * up, 0)
        y = np.where(ok, y + h[k] * x[i], y)
    return y


def peak_of(y):
    """(y32, peak): the float32 rounding and its largest magnitude (0 for an empty utterance)."""
    y32 = np.asarray(y, dtype=np.float64).astype(np.float32)
    return y32, np.float32(np.abs(y32).max(initial=0.0))


def to_int16(y32, peak, max_wav_value=MAX_WAV_VALUE):
    """The header's rule: trunc((y32 / peak) * max_wav_value) in float32, saturated; zeros for peak 0."""
    y32 = np.asarray(y32, dtype=np.float32)
    if not peak > 0:
        return np.zeros(len(y32), dtype=np.int16)
    v = (y32 / np.float32(peak)) * np.float32(max_wav_value)
    assert v.dtype == np.float32
    return np.clip(np.trunc(v), -32768.0, 32767.0).astype(np.int16)


def prepare(x, up, down, h, max_wav_value=MAX_WAV_VALUE):
    """(y, y32, peak, int16 row) of one utterance."""
    y = resample(x, up, down, h)
    y32, peak = peak_of(y)
    return y, y32, peak, to_int16(y32, peak, max_wav_value)


def pack(arrays, dtype):
    lens = np.array([len(a) for a in arrays], dtype=np.int64)
    out = np.zeros((len(arrays), max(int(lens.max(initial=0)), 1)), dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out, lens


def cases_of(fx, up, down):
    """The int16 cases of a ratio: (names, list of waveforms, list of scipy's outputs)."""
    k = key(up, down)
    names = [str(s) for s in fx["names_" + k]]
    wavs = [fx["wav_" + k][b, :n] for b, n in enumerate(fx["lens_" + k])]
    ys = [fx["y_" + k][b, :out_len(int(n), up, down)] for b, n in enumerate(fx["lens_" + k])]
    return names, wavs, ys
