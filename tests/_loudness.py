"""include/fs2hip_iir.h restated in plain numpy, operation for operation: the tables, the blocked
second-order sections with their Kogge-Stone scan, the state after the last sample, the BS.1770 gating
in the leaf-and-tree order of tests/_vad.py, and the gain (numpy has no fused multiply-add; every
expression below is one rounded float64 operation per operator). Also an np.longdouble direct
recurrence with plain gating, which the restatement is measured against, and the cases the loudness
tests share with tests/golden/gen_golden_loudness.py.
"""
import math
import os

import numpy as np

from _vad import LEAF, tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK, CHUNK, TABLE_LEN, S_MAX = 64, 16384, 412, 8  # FS2_IIR_BLOCK, _CHUNK, _TABLE_LEN, _S_MAX
RATES = (16000, 22050, 24000, 44100, 48000)
OFFSET, ABS_LUFS, REL_FACTOR = -0.691, -70.0, 0.1


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "loudness_a.npz")))


# ---- the K-weighting (fs2amd.audio.k_weighting_sos restated) and the tables ------------------------------

def k_weighting(fs):
    def tail(f0, Q):
        K = math.tan(math.pi * f0 / fs)
        return K, 1.0 + K / Q + K * K

    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K, a0 = tail(f0, Q)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    Q = 0.5003270373238773
    K, a0 = tail(38.13547087602444, Q)
    return np.array([shelf, [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]])


def _mm(A, B):
    """Row-major 2x2 product: two products and one add per element."""
    return np.array([A[0] * B[0] + A[1] * B[2], A[0] * B[1] + A[1] * B[3], A[2] * B[0] + A[3] * B[2],
                     A[2] * B[1] + A[3] * B[3]])


def section_tables(sec):
    """dict(p, q, P [6, 4], Q [65, 4]) of one section (rule 3)."""
    a1, a2 = np.float64(sec[4]), np.float64(sec[5])
    resp, end = [], []
    for z1, z2 in ((1.0, 0.0), (0.0, 1.0)):
        z1, z2 = np.float64(z1), np.float64(z2)
        ys = np.empty(BLOCK)
        for i in range(BLOCK):
            y = z1
            z1 = z2 - a1 * y
            z2 = -(a2 * y)
            ys[i] = y
        resp.append(ys)
        end.append((z1, z2))
    M = np.array([end[0][0], end[1][0], end[0][1], end[1][1]])
    P = [M]
    for _ in range(5):
        P.append(_mm(P[-1], P[-1]))
    Q = [np.array([1.0, 0.0, 0.0, 1.0])]
    for _ in range(BLOCK):
        Q.append(_mm(M, Q[-1]))
    return dict(p=resp[0], q=resp[1], P=np.array(P), Q=np.array(Q))


def tables(sos):
    """float64 [S, 412] in the layout of the header: what fs2amd.ops.sos_tables returns."""
    out = []
    for sec in np.asarray(sos, dtype=np.float64):
        t = section_tables(sec)
        out.append(np.concatenate([t["p"], t["q"], t["P"].ravel(), t["Q"].ravel()]))
    return np.array(out)


def _mv(A, v):
    """(A v) for v [..., 2]: two products and one add per component."""
    return np.stack([A[0] * v[..., 0] + A[1] * v[..., 1], A[2] * v[..., 0] + A[3] * v[..., 1]], axis=-1)


def section(x, sec, carry0):
    """One section over one row x (float64 [n], n >= 1): (y, zf) by rules 2, 4, 5 and 6."""
    b0, b1, b2, _, a1, a2 = (np.float64(c) for c in sec)
    t = section_tables(sec)
    n = len(x)
    nb = (n + BLOCK - 1) // BLOCK
    xp = np.zeros(nb * BLOCK)
    xp[:n] = x
    xp = xp.reshape(nb, BLOCK)
    length = np.minimum(n - BLOCK * np.arange(nb), BLOCK)
    # rule 2, every block at once; a block's state stops moving behind its last sample
    y0 = np.empty((nb, BLOCK))
    z1, z2 = np.zeros(nb), np.zeros(nb)
    for i in range(BLOCK):
        xv = xp[:, i]
        yv = b0 * xv + z1
        n1 = (b1 * xv - a1 * yv) + z2
        n2 = b2 * xv - a2 * yv
        live = i < length
        z1, z2 = np.where(live, n1, z1), np.where(live, n2, z2)
        y0[:, i] = yv
    c = np.stack([z1, z2], axis=1)
    # rule 4
    s = np.empty((nb, 2))
    carry = np.array(carry0, dtype=np.float64)
    for g0 in range(0, nb, 64):
        v = np.zeros((64, 2))
        m = min(64, nb - g0)
        v[:m] = c[g0:g0 + m]
        for j in range(6):
            d = 1 << j
            nv = v.copy()
            nv[d:] = _mv(t["P"][j], v[:-d]) + v[d:]
            v = nv
        s[g0] = carry
        for i in range(1, m):
            s[g0 + i] = _mv(t["Q"][i], carry) + v[i - 1]
        carry = _mv(t["Q"][64], carry) + v[63]
    # rule 5
    y = ((y0 + t["p"][None, :] * s[:, 0:1]) + t["q"][None, :] * s[:, 1:2]).reshape(-1)[:n]
    # rule 6
    w = b2 * x[n - 2] - a2 * y[n - 2] if n >= 2 else np.float64(carry0[1])
    zf = np.array([(b1 * x[n - 1] - a1 * y[n - 1]) + w, b2 * x[n - 1] - a2 * y[n - 1]])
    return y, zf


def sosfilt(x, sos, zi=None):
    """One row (int16 / float32 / float64 [n]) through all sections: (y float64 [n], zf [S, 2])."""
    sos = np.asarray(sos, dtype=np.float64)
    y = np.asarray(x).astype(np.float64)
    zi = np.zeros((len(sos), 2)) if zi is None else np.asarray(zi, dtype=np.float64)
    zf = zi.copy()
    if len(y) == 0:
        return y, zf
    with np.errstate(all="ignore"):
        for k, sec in enumerate(sos):
            y, zf[k] = section(y, sec, zi[k])
    return y, zf


def sosfilt_ld(x, sos):
    """The direct recurrence in np.longdouble (no blocks): what the restatement's error is measured against."""
    y = np.asarray(x).astype(np.longdouble)
    for sec in np.asarray(sos, dtype=np.float64):
        b0, b1, b2, _, a1, a2 = (np.longdouble(c) for c in sec)
        out = np.empty_like(y)
        z1 = z2 = np.longdouble(0)
        for i, xv in enumerate(y):
            yv = b0 * xv + z1
            z1 = b1 * xv - a1 * yv + z2
            z2 = b2 * xv - a2 * yv
            out[i] = yv
        y = out
    return y


# ---- the gate ---------------------------------------------------------------------------------------------

def gate_hop(fs):
    return int(round(fs / 10.0))


def blocks(n, H):
    return 0 if n < 4 * H else (n - 4 * H) // H + 1


def abs_gate(dtype):
    fsc = 32768.0 if np.dtype(dtype) == np.int16 else 1.0
    return 10.0 ** ((ABS_LUFS - OFFSET) / 10.0) * fsc ** 2


def target_z(lufs, dtype):
    fsc = 32768.0 if np.dtype(dtype) == np.int16 else 1.0
    return 10.0 ** ((float(lufs) - OFFSET) / 10.0) * fsc ** 2


def lufs_of(zbar, dtype):
    fsc = 32768.0 if np.dtype(dtype) == np.int16 else 1.0
    return -math.inf if not zbar > 0.0 else OFFSET + 10.0 * math.log10(float(zbar) / fsc ** 2)


def block_powers(y, H):
    """z_j float64 [J] of a filtered row in the header's order."""
    y = np.asarray(y, dtype=np.float64)
    J = blocks(len(y), H)
    if J == 0:
        return np.zeros(0)
    sq = (y[:(J + 3) * H] * y[:(J + 3) * H]).reshape(J + 3, H)
    leaves = np.stack([np.cumsum(sq[:, i:i + LEAF], axis=1)[:, -1] for i in range(0, H, LEAF)], axis=1)  # sequential
    S = tree(leaves)
    return ((S[0:J] + S[1:J + 1]) + (S[2:J + 2] + S[3:J + 3])) / np.float64(4 * H)


def gate(y, H, gate_abs, rel_factor=REL_FACTOR):
    """(zbar, (J, |A|, |R|)) of a filtered row."""
    z = block_powers(y, H)
    J = len(z)
    if J == 0:
        return 0.0, (0, 0, 0)
    A = z > np.float64(gate_abs)
    nA = int(A.sum())
    if nA == 0:
        return 0.0, (J, 0, 0)
    mean_a = tree(np.where(A, z, 0.0)) / np.float64(nA)
    R = A & (z > np.float64(rel_factor) * mean_a)
    nR = int(R.sum())
    if nR == 0:
        return 0.0, (J, nA, 0)
    return float(tree(np.where(R, z, 0.0)) / np.float64(nR)), (J, nA, nR)


def gate_plain(y, H, gate_abs, rel_factor=REL_FACTOR):
    """The same rule on any float type with numpy's own sums: (zbar, z, A, R, mean_A)."""
    J = blocks(len(y), H)
    if J == 0:
        return 0.0, np.zeros(0), None, None, None
    z = np.array([np.sum(y[j * H:j * H + 4 * H] ** 2) / (4 * H) for j in range(J)])
    A = z > gate_abs
    if not A.any():
        return 0.0, z, A, A, None
    mean_a = z[A].mean()
    R = A & (z > rel_factor * mean_a)
    return (z[R].mean() if R.any() else 0.0), z, A, R, mean_a


def measure(x, fs):
    """(zbar, counts) of an int16 / float32 row at rate fs, as fs2amd.loudness measures it."""
    y, _ = sosfilt(x, k_weighting(fs))
    return gate(y, gate_hop(fs), abs_gate(np.asarray(x).dtype))


# ---- the gain ---------------------------------------------------------------------------------------------

def gain(x, zbar, tz, peak_ceiling=0.0):
    """dict(q, gain, clipped, unmeasured, peak) of one int16 / float32 row."""
    x = np.asarray(x)
    v = x.astype(np.float64)
    peak = float(np.abs(v).max(initial=0.0))
    g, unmeasured = np.float64(1.0), 1
    if zbar > 0.0:
        g, unmeasured = np.sqrt(np.float64(tz) / np.float64(zbar)), 0
        if peak_ceiling > 0.0 and peak > 0.0:
            lim = np.float64(peak_ceiling) / np.float64(peak)
            g = lim if g > lim else g
    w = v * g
    if x.dtype == np.int16:
        r = np.rint(w)  # ties to even
        clipped = int(((r > 32767.0) | (r < -32768.0)).sum())
        q = np.clip(r, -32768.0, 32767.0).astype(np.int16)
    else:
        clipped, q = 0, w.astype(np.float32)
    return dict(q=q, gain=float(g), clipped=clipped, unmeasured=unmeasured, peak=peak)


def normalize(x, fs, target_lufs=-23.0, peak_ceiling=None):
    """dict(zbar, counts, lufs, + gain's) of one row, as fs2amd.normalize_loudness does it."""
    x = np.asarray(x)
    fsc = 32768.0 if x.dtype == np.int16 else 1.0
    zbar, counts = measure(x, fs)
    r = gain(x, zbar, target_z(target_lufs, x.dtype), 0.0 if peak_ceiling is None else peak_ceiling * fsc)
    return dict(r, zbar=zbar, counts=counts, lufs=lufs_of(zbar, x.dtype))


def pack(arrays, dtype):
    lens = np.array([len(a) for a in arrays], dtype=np.int64)
    out = np.zeros((len(arrays), max(int(lens.max(initial=0)), 1)), dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out, lens


# ---- the shared cases -------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.RandomState(seed)


def noise_i16(n, seed, amp=3000.0):
    return np.clip(np.round(_rng(seed).standard_normal(n) * amp), -32768, 32767).astype(np.int16)


def speech_row(n, fs, seed, dtype=np.int16, amp=2000.0):
    """Bursts of a voiced tone plus noise between silences: both gates have something to remove."""
    t = np.arange(n) / fs
    env = (np.sin(2 * np.pi * 0.7 * t) > 0.2) * np.abs(np.sin(2 * np.pi * 3 * t))
    x = env * (amp * np.sin(2 * np.pi * 180 * t) + 0.4 * amp * _rng(seed).standard_normal(n))
    if dtype == np.int16:
        return np.round(x).astype(np.int16)
    return (x / 32768.0 * np.float32(1.00037)).astype(np.float32)


def two_level_row(fs, seed=3, loud=6000.0, quiet=60.0):
    """3 s: a loud second, a quiet second 40 dB down (over the absolute gate, under the relative one), and
    a second of digital silence (under the absolute gate)."""
    g = _rng(seed)
    x = np.concatenate([g.standard_normal(fs) * loud, g.standard_normal(fs) * quiet, np.zeros(fs)])
    return np.round(x).astype(np.int16)


def sine_row(fs, seconds=3.0, f=997.0, amp=32767.0):
    return np.round(amp * np.sin(2 * np.pi * f * np.arange(int(fs * seconds)) / fs)).astype(np.int16)


SOS_LENGTHS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193, 3 * 4096 + 17, 16384, 16385, 2 * 16384 + 1)


def hostile_sos():
    """name -> (sos, fs): sections with poles close to the unit circle."""
    from scipy import signal

    return {"hp20": (signal.butter(4, 20, "hp", fs=48000, output="sos"), 48000),
            "bp300_3400": (signal.butter(6, [300, 3400], "bp", fs=16000, output="sos"), 16000),
            "notch50_r0999": (np.array([[1.0, -2.0 * math.cos(2 * math.pi * 50 / 48000), 1.0, 1.0,
                                         -2.0 * 0.9995 * math.cos(2 * math.pi * 50 / 48000), 0.9995 ** 2]]), 48000)}


def sections_for(S):
    """S sections for the sosfilt tests: K-weighting at 22050 for 2, its shelf for 1, Butterworth cascades beyond."""
    from scipy import signal

    if S == 1:
        return k_weighting(22050)[:1]
    if S == 2:
        return k_weighting(22050)
    if S == 3:
        return signal.butter(6, 0.2, "lp", output="sos")
    return signal.butter(2 * S, [0.1, 0.6], "bp", output="sos")[:S]


def fixture_cases():
    """name -> (row, fs): every row whose measurements the fixture records."""
    cases = {}
    for fs in (16000, 22050):
        cases[f"speech_i16_{fs}"] = (speech_row(int(1.3 * fs), fs, 31), fs)
        cases[f"speech_f32_{fs}"] = (speech_row(int(1.1 * fs), fs, 32, np.float32), fs)
    cases["two_level_8000"] = (two_level_row(8000), 8000)
    cases["short_22050"] = (noise_i16(4 * 2205 - 1, 33), 22050)
    cases["silent_22050"] = (np.zeros(3 * 2205 * 4, dtype=np.int16), 22050)
    return cases
