"""float64 numpy restatements of include/fs2hip_align.h — monotonic alignment search and the
forward-sum (CTC) loss with its gradient — the case table of the alignment tests, and the loader of
tests/golden/align_a.npz (written by tests/golden/gen_golden_align.py)."""
import itertools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_a.npz")

# (T_b, L_b) of the ragged batch: a single cell; L = 1; T = L (only the diagonal is feasible), twice;
# L one past a wavefront (65 phonemes, 131 CTC states); T beyond two bitmap words
CASES = ((1, 1), (5, 1), (3, 3), (7, 3), (33, 17), (64, 64), (70, 65), (130, 9))
T_MAX, L_MAX = 136, 70
BLANK = -1.0
NINF = -np.inf


def make_logp(T, L, seed):
    """Attention log-probabilities as an aligner emits them: log_softmax over the phonemes of
    2 * N(0, 1) scores, float64 [T, L]."""
    x = 2.0 * np.random.default_rng(seed).standard_normal((T, L))
    x = x - x.max(axis=1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=1, keepdims=True))


def batch_logp(dtype=np.float64):
    """The ragged batch [B, T_MAX, L_MAX] with NaN outside every utterance's [T_b, L_b], and the per-
    utterance matrices. float32: the float64 values rounded once (the kernels widen them exactly)."""
    mats = [make_logp(T, L, 100 + i).astype(dtype) for i, (T, L) in enumerate(CASES)]
    full = np.full((len(CASES), T_MAX, L_MAX), np.nan, dtype=dtype)
    for b, m in enumerate(mats):
        full[b, :m.shape[0], :m.shape[1]] = m
    return full, mats


def mas_ref(x):
    """x [T, L] (any float dtype; widened to float64) -> (durations int64 [L], score float64, path
    int32 [T]); None durations / path and -inf when T < L or a length is 0."""
    x = np.asarray(x, dtype=np.float64)
    T, L = x.shape
    if T == 0 or L == 0 or T < L:
        return None, NINF, None
    v = np.full(L, NINF)
    v[0] = x[0, 0]
    dec = np.zeros((T, L), dtype=bool)
    for t in range(1, T):
        vd = np.concatenate(([NINF], v[:-1]))
        d = vd >= v
        d[0] = False
        dec[t] = d
        v = x[t] + np.where(d, vd, v)
    dur = np.zeros(L, dtype=np.int64)
    path = np.zeros(T, dtype=np.int32)
    j = L - 1
    for t in range(T - 1, -1, -1):
        dur[j] += 1
        path[t] = j
        if t >= 1 and dec[t, j]:
            j -= 1
    return dur, v[L - 1], path


def mas_brute(x):
    """The best monotonic path by enumeration: (score, the set of duration tuples that reach it).
    A path's score is summed in frame order, as the recurrence does."""
    x = np.asarray(x, dtype=np.float64)
    T, L = x.shape
    best, arg = NINF, set()
    for cuts in itertools.combinations(range(1, T), L - 1):
        edges = (0,) + cuts + (T,)
        dur = tuple(edges[i + 1] - edges[i] for i in range(L))
        s, t = None, 0
        for j, d in enumerate(dur):
            for _ in range(d):
                s = x[t, j] if s is None else x[t, j] + s
                t += 1
        if s > best:
            best, arg = s, {dur}
        elif s == best:
            arg.add(dur)
    return best, arg


def _lse(*a):
    m = max(a)
    if m == NINF:
        m = 0.0
    s = np.exp(a[0] - m) + np.exp(a[1] - m)
    for v in a[2:]:
        s = s + np.exp(v - m)
    return np.log(s) + m


def log_softmax_blank(x, blank=BLANK):
    """lp [T, L + 1] of the header: class 0 is the blank."""
    x = np.asarray(x, dtype=np.float64)
    z = np.concatenate([np.full((x.shape[0], 1), blank), x], axis=1)
    m = z.max(axis=1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def forward_sum_ref(x, blank=BLANK):
    """x [T, L] -> (nll, d nll / d x [T, L], alpha [T, 2 L + 1]) in float64, the header's operation
    order; (inf, zeros, None) when T < L or a length is 0."""
    x = np.asarray(x, dtype=np.float64)
    T, L = x.shape
    if T == 0 or L == 0 or T < L:
        return np.inf, np.zeros((T, L)), None
    lp = log_softmax_blank(x, blank)
    S = 2 * L + 1
    cls = [0 if s % 2 == 0 else (s + 1) // 2 for s in range(S)]
    with np.errstate(divide="ignore"):
        alpha = np.full((T, S), NINF)
        alpha[0, 0], alpha[0, 1] = lp[0, 0], lp[0, 1]
        for t in range(1, T):
            for s in range(S):
                a2 = alpha[t - 1, s - 1] if s >= 1 else NINF
                a3 = alpha[t - 1, s - 2] if s % 2 == 1 and s >= 3 else NINF
                alpha[t, s] = _lse(alpha[t - 1, s], a2, a3) + lp[t, cls[s]]
        nll = -_lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2])
        beta = np.full((T, S), NINF)
        beta[T - 1, S - 1], beta[T - 1, S - 2] = lp[T - 1, 0], lp[T - 1, L]
        for t in range(T - 2, -1, -1):
            for s in range(S):
                b2 = beta[t + 1, s + 1] if s + 1 < S else NINF
                b3 = beta[t + 1, s + 2] if s % 2 == 1 and s + 2 < S else NINF
                beta[t, s] = _lse(beta[t + 1, s], b2, b3) + lp[t, cls[s]]
        if not np.isfinite(nll):
            return np.inf, np.zeros((T, L)), alpha
        grad = np.zeros((T, L))
        for j in range(L):
            s = 2 * j + 1
            grad[:, j] = np.exp(lp[:, j + 1]) - np.exp(((alpha[:, s] + beta[:, s]) + nll) - lp[:, j + 1])
    return nll, grad, alpha


def path_matrix(dur, T, L, on=0.0, off=-20.0):
    """[T, L]: ``on`` along the path of the durations ``dur``, ``off`` elsewhere."""
    x = np.full((T, L), off)
    t = 0
    for j, d in enumerate(dur):
        x[t:t + d, j] = on
        t += d
    assert t == T
    return x


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
