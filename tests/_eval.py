"""float64 numpy restatements of include/fs2hip_eval.h — mel cepstra, pairwise distances, dynamic
time warping and the statistics along its path — the case table of the evaluation tests, and the
loader of tests/golden/eval_a.npz (written by tests/golden/gen_golden_eval.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "eval_a.npz")

# (Tx_b, Ty_b) of the ragged batch: a single cell; one row; one column; a square; a short one; past a
# ballot word on neither side, on both, one past it; a long x against a short y and the other way
# round (the tie rule is stated in the caller's (i, j)); more than 256 cells on an anti-diagonal
CASES = ((1, 1), (1, 5), (5, 1), (3, 3), (7, 4), (33, 17), (64, 64), (65, 70), (130, 9), (9, 130), (300, 270))
TX_MAX, TY_MAX, D = 300, 270, 13
N_MEL, N_COEF = 80, 13
ALPHA = 6.141851463713754  # 10 / ln 10 * sqrt 2
INF = np.inf


def make_feats(T, Dx, seed):
    """Continuous random frames with a slow drift, float64 [T, Dx]: no two costs tie."""
    rng = np.random.default_rng(seed)
    return np.cumsum(0.3 * rng.standard_normal((T, Dx)), axis=0) + rng.standard_normal((T, Dx))


def batch_feats(dtype=np.float64):
    """The ragged batch: x [B, TX_MAX, D] and y [B, TY_MAX, D] with NaN outside every utterance's own
    frames, and the per-utterance matrices. float32: the float64 values rounded once."""
    xs = [make_feats(Tx, D, 300 + 2 * b).astype(dtype) for b, (Tx, _) in enumerate(CASES)]
    ys = [make_feats(Ty, D, 301 + 2 * b).astype(dtype) for b, (_, Ty) in enumerate(CASES)]
    x = np.full((len(CASES), TX_MAX, D), np.nan, dtype=dtype)
    y = np.full((len(CASES), TY_MAX, D), np.nan, dtype=dtype)
    for b in range(len(CASES)):
        x[b, :xs[b].shape[0]] = xs[b]
        y[b, :ys[b].shape[0]] = ys[b]
    return x, y, xs, ys


def make_mel(T, seed, n_mel=N_MEL):
    """Log-mel frames as the model's targets range: uniform in [-11.5, 2], float64 [T, n_mel]."""
    return np.random.default_rng(seed).uniform(-11.5, 2.0, (T, n_mel))


def make_f0(T, seed):
    """An F0 contour in Hz with unvoiced stretches (0), float64 [T]."""
    rng = np.random.default_rng(seed)
    f0 = 180.0 * 2.0 ** (0.3 * np.sin(np.arange(T) / 7.0 + rng.uniform(0, 6)) + 0.05 * rng.standard_normal(T))
    voiced = np.sin(np.arange(T) / 5.0 + rng.uniform(0, 6)) > -0.3
    return np.where(voiced, f0, 0.0)


def dct_basis(n_mel=N_MEL, n_coef=N_COEF):
    """Rows 1 .. n_coef of the orthonormal DCT-II, float64 [n_coef, n_mel]."""
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    q = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    return np.sqrt(2.0 / n_mel) * np.cos(np.pi / n_mel * (m + 0.5) * q)


def mel_cepstrum_ref(mel, basis):
    """mel [T, M] (widened to float64), basis [C, M] -> [T, C]: s = s + mel[t, m] * basis[q, m] for
    m = 0 .. M-1 from zero, one multiplication and one addition each."""
    mel = np.asarray(mel, dtype=np.float64)
    s = np.zeros((mel.shape[0], basis.shape[0]))
    for m in range(mel.shape[1]):
        s = s + mel[:, m:m + 1] * basis[None, :, m]
    return s


def pair_sq_ref(x, y):
    """s[i, j] = sum_d (x[i, d] - y[j, d])^2 in index order from zero, float64 [Tx, Ty]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s = np.zeros((x.shape[0], y.shape[0]))
    for d in range(x.shape[1]):
        e = x[:, d:d + 1] - y[None, :, d]
        s = s + e * e
    return s


def pair_dist_ref(x, y):
    return np.sqrt(pair_sq_ref(x, y))


def dtw_from_cost(c):
    """The recursion and the backtrack of the header over a cost matrix c [Tx, Ty], one anti-diagonal
    at a time -> (total float64, K int, path_i int32 [K], path_j int32 [K]) in forward order."""
    c = np.asarray(c, dtype=np.float64)
    Tx, Ty = c.shape
    A = np.full((Tx + 1, Ty + 1), INF)  # A[i + 1, j + 1] is the header's A[i, j]
    step = np.zeros((Tx, Ty), dtype=np.uint8)
    A[1, 1] = c[0, 0]
    for e in range(1, Tx + Ty - 1):
        i = np.arange(max(0, e - (Ty - 1)), min(e, Tx - 1) + 1)
        j = e - i
        p, u, l = A[i, j], A[i, j + 1], A[i + 1, j]
        s = np.where((p <= u) & (p <= l), 0, np.where(u <= l, 1, 2)).astype(np.uint8)
        step[i, j] = s
        A[i + 1, j + 1] = c[i, j] + np.where(s == 0, p, np.where(s == 1, u, l))
    i, j = Tx - 1, Ty - 1
    pi, pj = [i], [j]
    while i or j:
        s = step[i, j]
        i, j = i - (s != 2), j - (s != 1)
        pi.append(i)
        pj.append(j)
    return A[Tx, Ty], len(pi), np.array(pi[::-1], dtype=np.int32), np.array(pj[::-1], dtype=np.int32)


def dtw_ref(x, y):
    """The pure-host restatement: numpy's costs, then the recursion."""
    return dtw_from_cost(pair_dist_ref(x, y))


def dtw_brute(c):
    """Every warping path from (0, 0) to the end by steps (1, 1), (1, 0), (0, 1): (the least total,
    summed from the start of the path, the set of paths that reach it as tuples of (i, j))."""
    c = np.asarray(c, dtype=np.float64)
    Tx, Ty = c.shape
    best, arg = INF, set()
    stack = [((0, 0),)]
    while stack:
        path = stack.pop()
        i, j = path[-1]
        if (i, j) == (Tx - 1, Ty - 1):
            tot = 0.0
            for a, b in path:
                tot = tot + c[a, b]
            if tot < best - 1e-12:
                best, arg = tot, {path}
            elif abs(tot - best) <= 1e-12:
                arg.add(path)
            continue
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Tx and j + dj < Ty:
                stack.append(path + ((i + di, j + dj),))
    return best, arg


def padded_path(K, pi, pj, width):
    """(path_i, path_j) as the kernel writes one utterance's rows: int32 [width], -1 from K on."""
    oi = np.full(width, -1, dtype=np.int32)
    oj = np.full(width, -1, dtype=np.int32)
    oi[:K], oj[:K] = pi, pj
    return oi, oj


def path_stats_ref(a, b, pi, pj, K):
    """a [Tx, Ch], b [Ty, Ch] float64 with NaN = absent, along the first K path entries ->
    (counts int64 [Ch, 4] = both, a only, b only, none; sums float64 [Ch, 2] = sum d, sum d^2 over the
    both-present pairs in path order from zero)."""
    Ch = a.shape[1]
    counts = np.zeros((Ch, 4), dtype=np.int64)
    sums = np.zeros((Ch, 2))
    for ch in range(Ch):
        s = s2 = 0.0
        for k in range(K):
            va, vb = a[pi[k], ch], b[pj[k], ch]
            ha, hb = not np.isnan(va), not np.isnan(vb)
            if ha and hb:
                d = va - vb
                s = s + d
                s2 = s2 + d * d
            counts[ch, 0 if ha and hb else 1 if ha else 2 if hb else 3] += 1
        sums[ch] = s, s2
    return counts, sums


def f0_tracks(f0):
    """The two channels f0_metrics reads: Hz and cents (1200 log2), NaN where unvoiced; [T, 2]."""
    f0 = np.asarray(f0, dtype=np.float64)
    hz = np.where(f0 > 0, f0, np.nan)
    with np.errstate(invalid="ignore"):
        return np.stack((hz, 1200.0 * np.log2(hz)), axis=-1)


def load_golden():
    return np.load(GOLDEN)
