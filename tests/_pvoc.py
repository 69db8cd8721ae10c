"""The numpy restatement of include/fs2hip_pvoc.h (the phase vocoder as a running product of unit rotors,
float64, nothing contracted: numpy rounds every ufunc on its own), vectorised over bins and lanes; the
angle form of librosa.phase_vocoder in float64 for comparison; the input rows of the tests and of
tests/golden/pvoc_a.npz."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 64          # FS2_PVOC_BLOCK
J_CAP = 2 ** 31 - 1  # FS2_PVOC_J_CAP
SEMITONE = 2.0 ** (1.0 / 12.0)
KERNEL_T = (0, 1, 2, 63, 64, 65, 130)
KERNEL_RATES = (0.25, 0.5, 1.0, SEMITONE, 1.5, 2.0, 3.7)


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "pvoc_a.npz")))


def frames(T, rate):
    """Rule 1: the number of j >= 0 with fl(j * rate) < T (saturated at J_CAP); 0 for an invalid rate."""
    T, rate = int(T), float(rate)
    if T < 1 or not rate > 0.0 or not math.isfinite(rate):
        return 0
    t = float(min(T, J_CAP))
    q = t / rate
    if not q < 2147483649.0:
        return J_CAP
    j = math.ceil(q)
    while j > 0 and not float(j - 1) * rate < t:
        j -= 1
    while float(j) * rate < t:
        j += 1
    return min(j, J_CAP)


def frames_by_definition(T, rate, limit=1 << 16):
    """The same count by trying every j below limit."""
    if not (rate > 0.0 and math.isfinite(rate)):
        return 0
    n = int((np.arange(limit, dtype=np.float64) * np.float64(rate) < T).sum())
    assert n < limit
    return n


def cmul(a, b):
    """(x, y) (*) (u, v) = (x u - y v, x v + y u) on pairs of arrays."""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def units(spec, T):
    """Rule 2 over a row's first T frames plus the zero pad: m [NB, T + 1], (ex, ey) likewise."""
    NB = spec.shape[0] // 2
    re, im = spec[:NB, :T].astype(np.float64), spec[NB:, :T].astype(np.float64)
    m = np.sqrt(re * re + im * im)
    zero = m == 0.0
    safe = np.where(zero, 1.0, m)
    ex, ey = np.where(zero, 1.0, re / safe), np.where(zero, 0.0, im / safe)
    pad0, pad1 = np.zeros((NB, 1)), np.ones((NB, 1))
    return np.concatenate([m, pad0], 1), np.concatenate([ex, pad1], 1), np.concatenate([ey, pad0], 1)


def scan(sx, sy):
    """Rule 4: the inclusive prefix of (sx, sy) [NB, J] under (*) in the header's order."""
    NB, J = sx.shape
    nblk = -(-J // BLOCK)
    x, y = np.ones((NB, nblk * BLOCK)), np.zeros((NB, nblk * BLOCK))
    x[:, :J], y[:, :J] = sx, sy
    x, y = x.reshape(NB, nblk, BLOCK), y.reshape(NB, nblk, BLOCK)
    d = 1
    while d < BLOCK:  # Kogge-Stone inside every block at once
        nx, ny = cmul((x[:, :, :-d], y[:, :, :-d]), (x[:, :, d:], y[:, :, d:]))
        x, y = np.concatenate([x[:, :, :d], nx], 2), np.concatenate([y[:, :, :d], ny], 2)
        d *= 2
    for c in range(1, nblk):  # the carry: the last element of the block before
        x[:, c], y[:, c] = cmul((x[:, c - 1, -1:], y[:, c - 1, -1:]), (x[:, c], y[:, c]))
    return x.reshape(NB, -1)[:, :J], y.reshape(NB, -1)[:, :J]


def pvoc64(spec, T, rate):
    """One row in float64: (mag [NB, J], Px, Py). spec f32 [2 NB, >= T]."""
    spec = np.asarray(spec)
    assert spec.dtype == np.float32 and spec.ndim == 2 and spec.shape[0] % 2 == 0
    NB = spec.shape[0] // 2
    T = min(max(int(T), 0), spec.shape[1])
    J = frames(T, rate)
    if J == 0:
        z = np.zeros((NB, 0))
        return z, z, z
    m, ex, ey = units(spec, T)
    p = np.arange(J, dtype=np.float64) * np.float64(rate)
    i = np.floor(p).astype(np.int64)
    assert i[-1] <= T - 1
    alpha = p - i
    mag = (1.0 - alpha) * m[:, i] + alpha * m[:, i + 1]
    a0, b0, a1, b1 = ex[:, i], ey[:, i], ex[:, i + 1], ey[:, i + 1]
    rx, ry = a1 * a0 + b1 * b0, b1 * a0 - a1 * b0
    sx, sy = np.concatenate([ex[:, :1], rx[:, :J - 1]], 1), np.concatenate([ey[:, :1], ry[:, :J - 1]], 1)
    Px, Py = scan(sx, sy)
    return mag, Px, Py


def pvoc(spec, T, rate):
    """One row as the kernel writes it: recomb f32 [2 NB, J] (rule 5)."""
    mag, Px, Py = pvoc64(spec, T, rate)
    return np.concatenate([(mag * Px).astype(np.float32), (mag * Py).astype(np.float32)], 0)


def pvoc_angle(spec, T, rate, hop=256):
    """librosa.phase_vocoder's rule in float64 with angles, over the time steps of rule 1:
    (out complex128 [NB, J], the largest |phase_acc| met)."""
    spec = np.asarray(spec)
    NB = spec.shape[0] // 2
    D = spec[:NB, :T].astype(np.float64) + 1j * spec[NB:, :T].astype(np.float64)
    J = frames(T, rate)
    out = np.zeros((NB, J), dtype=np.complex128)
    if J == 0:
        return out, 0.0
    D = np.concatenate([D, np.zeros((NB, 2), dtype=np.complex128)], 1)
    phi_advance = np.linspace(0.0, np.pi * hop, NB)
    phase_acc = np.angle(D[:, 0])
    biggest = float(np.abs(phase_acc).max())
    steps = np.arange(J, dtype=np.float64) * np.float64(rate)
    for t, step in enumerate(steps):
        c0, c1 = D[:, int(step)], D[:, int(step) + 1]
        alpha = np.mod(step, 1.0)
        mag = (1.0 - alpha) * np.abs(c0) + alpha * np.abs(c1)
        out[:, t] = mag * (np.cos(phase_acc) + 1j * np.sin(phase_acc))
        dphase = np.angle(c1) - np.angle(c0) - phi_advance
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        phase_acc = phase_acc + (phi_advance + dphase)
        biggest = max(biggest, float(np.abs(phase_acc).max()))
    return out, biggest


def rescale_durations(durations, rate, n_new, hop=256):
    """The duration rule of augment_utterances: c'_k = min(T', floor(c_k / rate + 0.5)) over the cumulative
    boundaries, T' = 1 + n_new // hop; the new durations are the differences."""
    c = np.cumsum(np.asarray(durations, dtype=np.int64))
    T_new = 1 + int(n_new) // hop
    cn = np.minimum(T_new, np.floor(c / float(rate) + 0.5).astype(np.int64))
    return np.diff(np.concatenate([[0], cn])).astype(np.int64)


def closest_fraction(f, limit=256):
    """(p, q) in lowest terms with max(p, q) <= limit and |p / q - f| least (the smallest q on a tie)."""
    best = None
    for q in range(1, limit + 1):
        for p in {min(max(int(math.floor(f * q)), 1), limit), min(max(int(math.floor(f * q)) + 1, 1), limit)}:
            err = abs(p / q - f)
            if best is None or err < best[0]:
                best = (err, p, q)
    g = math.gcd(best[1], best[2])
    return best[1] // g, best[2] // g


def stretch_len(n, rate):
    return int(round(n / rate))


def cut_pad(x, n):
    out = np.zeros(n, dtype=x.dtype)
    out[:min(n, len(x))] = x[:n]
    return out


# ---- inputs -----------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.default_rng(seed)


def random_spec(NB, T, seed, scale=1.0):
    """f32 [2 NB, T]: a slowly rotating partial per bin with noise on it, so that neighbouring frames are
    correlated as an STFT's are, none of it dyadic."""
    r = _rng(seed)
    t = np.arange(max(T, 1))[None, :]
    w = r.uniform(-3.0, 3.0, (NB, 1))
    amp = r.uniform(0.1, 2.0, (NB, 1)) * (1.0 + 0.5 * np.sin(0.11 * t + r.uniform(0, 6, (NB, 1))))
    z = amp * np.exp(1j * (w * t + r.uniform(0, 6, (NB, 1)))) + 0.2 * (r.standard_normal((NB, max(T, 1))) +
                                                                    1j * r.standard_normal((NB, max(T, 1))))
    z = (z * scale)[:, :T]
    return np.concatenate([z.real, z.imag], 0).astype(np.float32)


def zero_frames_spec(NB=5, T=40, seed=7):
    """Zero frames at the start, in the middle and at the end; bin 3 all zero."""
    s = random_spec(NB, T, seed)
    for a, b in ((0, 3), (17, 21), (T - 2, T)):
        s[:, a:b] = 0.0
    s[3] = 0.0
    s[NB + 3] = 0.0
    return s


def extreme_spec(NB=5, T=70, seed=9):
    """Exact-zero bins and f32 values of 1e-30 and 1e30 in one row."""
    s = random_spec(NB, T, seed)
    s[0, :] = 0.0                      # re = 0 everywhere: a purely imaginary bin
    s[1, ::3] = np.float32(1e30)
    s[NB + 1, 1::3] = np.float32(-1e30)
    s[2, :] = np.float32(1e-30) * s[2, :]
    s[NB + 2, :] = np.float32(1e-30) * s[NB + 2, :]
    s[4, 10:20] = 0.0
    s[NB + 4, 10:20] = 0.0             # exact zeros in both parts
    s[3, 30] = np.float32(1e30)
    s[NB + 3, 31] = np.float32(1e-30)
    return s


def kernel_cases(NB=5):
    """(name, spec, T, rate) over KERNEL_T x KERNEL_RATES, and one more row for J = 129 (one frame past two
    blocks), which that grid does not give."""
    cases = []
    for ti, T in enumerate(KERNEL_T):
        spec = random_spec(NB, T, 100 + ti)
        for ri, rate in enumerate(KERNEL_RATES):
            cases.append((f"k_{T}_{ri}", spec, T, rate))
    cases.append(("k_129_2", random_spec(NB, 129, 150), 129, 1.0))
    return cases


RAGGED_T = (130, 64, 0, 65, 33, 100, 1)
RAGGED_RATES = (0.25, SEMITONE, 1.0, 0.0, float("nan"), 3.7, 0.5)


def ragged_rows(NB=5):
    return [(random_spec(NB, T, 200 + b), T, r) for b, (T, r) in enumerate(zip(RAGGED_T, RAGGED_RATES))]


def fixture_cases():
    """name -> (spec, T, rate): every case whose output the fixture records."""
    cases = {name: (spec, T, rate) for name, spec, T, rate in kernel_cases()}
    for b, (spec, T, rate) in enumerate(ragged_rows()):
        cases[f"ragged_{b}"] = (spec, T, rate)
    cases["zero_frames_0.8"] = (zero_frames_spec(), 40, 0.8)
    cases["zero_frames_1.25"] = (zero_frames_spec(), 40, 1.25)
    cases["extreme_0.9"] = (extreme_spec(), 70, 0.9)
    cases["extreme_1.7"] = (extreme_spec(), 70, 1.7)
    return cases


def waveform(n, seed, dtype=np.float32):
    """A gliding harmonic tone with an envelope and a little noise."""
    r = _rng(seed)
    t = np.arange(n) / 22050.0
    f = 140.0 + 10.0 * seed + 30.0 * np.sin(2 * np.pi * 1.1 * t)
    ph = 2 * np.pi * np.cumsum(f) / 22050.0
    x = 0.3 * sum(np.sin(h * ph) / h for h in (1, 2, 3)) * (0.4 + 0.6 * np.abs(np.sin(5.0 * t + seed)))
    x = x + 0.01 * r.standard_normal(n)
    if dtype == np.int16:
        return np.round(x * 20000.0).astype(np.int16)
    return x.astype(np.float32)
