"""The F0 tracker of include/fs2hip_f0_track.h restated in plain numpy and Python: the oracle of the
tracker's tests. Nothing of the reference's exists to compare with (it takes F0 from pyworld), and
neither pyworld nor librosa is installed where this suite runs: the contract is the header's.

``Tables`` builds the host tables from exact rationals (``fractions``) and correctly rounded
logarithms (``decimal`` at 60 digits), so that they do not depend on a platform's libm.
``frame_candidates`` goes from one dp row to the frame's sparse observation, ``viterbi`` is dense
numpy over all 2 N states (no band loop per lane, no double buffer: not the kernel's structure),
``track`` chains the two for one utterance. ``fragile`` lists the comparisons of the candidate stage
that a rounding of dp could flip; ``fixture_faults`` checks what the fixture has to show.
"""
import decimal
import math
import os
from fractions import Fraction

import numpy as np

import _f0 as Y

GOLDEN = Y.GOLDEN
N_THR, BETA_A, BETA_B = 100, 2, 18
P_ABSENT = Fraction(1, 100)  # p_a of the header
P_FLOOR = Fraction(1, 10 ** 12)  # probability of a voiced bin without a candidate; floor of every other one
_CTX = decimal.Context(prec=60)
NEG_INF = float("-inf")


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "f0_track_a.npz")))


def _dec(q):
    q = Fraction(q)
    return _CTX.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))


def _log(q):
    """The double nearest ln(q) of an exact rational q > 0; -inf for q == 0."""
    return float(_CTX.ln(_dec(q))) if q > 0 else NEG_INF


class Tables:
    """The host tables of the header for one parameter set."""

    def __init__(self, sr=Y.SR, f0_floor=Y.F0_FLOOR, f0_ceil=Y.F0_CEIL, bins_per_semitone=5, max_step=12,
                 switch_prob=0.01):
        self.sr, self.f0_floor, self.f0_ceil = float(sr), float(f0_floor), float(f0_ceil)
        self.tau_min, self.tau_max = Y.lags(sr, f0_floor, f0_ceil)
        R, K = int(bins_per_semitone), int(max_step)
        self.R, self.K = R, K
        self.N = N = int(math.ceil(12 * R * math.log2(self.f0_ceil / self.f0_floor) - 1e-9))
        floor_log = _log(P_FLOOR)
        # thresholds s_i = i / 100 and the discretised Beta(2, 18) over them, exact
        self.S = np.array([i / N_THR for i in range(N_THR + 1)], dtype=np.float64)
        w = [Fraction(i, N_THR) ** (BETA_A - 1) * (1 - Fraction(i, N_THR)) ** (BETA_B - 1) for i in range(1, N_THR + 1)]
        z = sum(w)
        C = [Fraction(0)]
        for x in w:
            C.append(C[-1] + x / z)
        assert C[N_THR] == 1
        self.C = C
        pa = P_ABSENT
        n1 = N_THR + 1
        self.LM0 = np.full((n1, n1), NEG_INF)
        self.LM1 = np.full((n1, n1), NEG_INF)
        for u in range(n1):
            for v in range(u, n1):
                if C[v] - C[u] > 0:
                    self.LM0[u, v] = max(_log(C[v] - C[u]), floor_log)
                m1 = (C[v] - C[u]) + pa * C[u]
                if m1 > 0:
                    self.LM1[u, v] = max(_log(m1), floor_log)
        # unvoiced: what the thresholds without a candidate keep, spread over the N bins; [101]: no candidate
        self.LU = np.array([_log(max((1 - pa) * C[g] / N, P_FLOOR)) for g in range(n1)] + [_log(Fraction(1, N))])
        self.FLOOR = floor_log
        self.LINIT = _log(Fraction(1, 2 * N))
        sw = Fraction(switch_prob)
        tri = [Fraction(K + 1 - d, (K + 1) ** 2) for d in range(K + 1)]
        self.TS = np.array([_log(t * (1 - sw)) for t in tri])
        self.TX = np.array([_log(t * sw) for t in tri])
        # bin edges as periods: E[n] = sr / (f0_floor * 2^(n / (12 R))), decreasing
        two = decimal.Decimal(2)
        self.E = np.array([float(_CTX.divide(decimal.Decimal(self.sr), _CTX.multiply(
            decimal.Decimal(self.f0_floor), _CTX.power(two, _CTX.divide(decimal.Decimal(n), decimal.Decimal(12 * R))))))
            for n in range(N + 1)])
        assert (np.diff(self.E) < 0).all()

    def thr_index(self, dp):
        """a: the smallest i in 1..100 with dp < S[i], 101 when there is none (a NaN: none)."""
        for i in range(1, N_THR + 1):
            if dp < self.S[i]:
                return i
        return N_THR + 1

    def bin_of(self, p):
        """The number of n in 1..N-1 with p <= E[n]."""
        return int(sum(1 for n in range(1, self.N) if p <= self.E[n]))


_CACHE = {}


def tables(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CACHE:
        _CACHE[key] = Tables(**kw)
    return _CACHE[key]


def frame_candidates(dp, tb, trace=None):
    """One dp row [tau_max + 1] -> (cands, g): cands a list of (bin, log_mass, f, lag) in lag order,
    one per bin, log_mass > -inf; g the index into tb.LU. trace: receives (lhs, rhs, scale, kind)
    for every comparison that depends on dp, as tests/_f0.py: pick does."""
    dp = np.asarray(dp, dtype=np.float64)
    note = trace.append if trace is not None else (lambda c: None)
    found = []  # (lag, dp, p, f)
    for t in range(tb.tau_min, tb.tau_max):
        note((dp[t], dp[t - 1], max(abs(dp[t]), abs(dp[t - 1])), "dp"))
        note((dp[t], dp[t + 1], max(abs(dp[t]), abs(dp[t + 1])), "dp"))
        if not (dp[t] < dp[t - 1] and dp[t] <= dp[t + 1]):
            continue
        a, b, c = dp[t - 1], dp[t], dp[t + 1]
        den = (a - np.float64(2.0) * b) + c
        note((den, 0.0, abs(a) + 2 * abs(b) + abs(c), "dp"))
        with np.errstate(invalid="ignore", divide="ignore"):
            delta = (np.float64(0.5) * (a - c)) / den if den > 0 else np.float64(0.0)
            p = np.float64(t) + delta
            f = np.float64(tb.sr) / p
        note((f, tb.f0_floor, tb.f0_floor, "range"))
        note((f, tb.f0_ceil, tb.f0_ceil, "range"))
        if tb.f0_floor <= f <= tb.f0_ceil:
            found.append((t, float(dp[t]), float(p), float(f)))
    if not found:
        return [], N_THR + 1
    best = 0
    for c in range(1, len(found)):
        if found[c][1] < found[best][1]:
            best = c
    for c in range(len(found)):
        if c != best:
            note((found[c][1], found[best][1], max(abs(found[c][1]), abs(found[best][1])), "dpmin"))
    m = N_THR + 1
    per_bin = {}
    for c, (t, d, p, f) in enumerate(found):
        a = tb.thr_index(d)
        if a <= N_THR:
            note((d, tb.S[a], tb.S[a], "dp"))
        if a > 1:
            note((d, tb.S[a - 1], max(abs(d), tb.S[a - 1]), "dp"))
        u = a - 1
        if c == best:
            lm = tb.LM1[u, m - 1]
        else:
            lm = tb.LM0[u, m - 1] if a < m else NEG_INF
        m = min(m, a)
        if not lm > NEG_INF:
            continue
        n = tb.bin_of(p)
        if n + 1 <= tb.N:
            note((p, tb.E[n + 1], tb.E[n + 1], "range"))
        if n >= 1:
            note((p, tb.E[n], tb.E[n], "range"))
        if n not in per_bin or lm > per_bin[n][1]:  # a tie keeps the smaller lag
            per_bin[n] = (n, float(lm), f, t)
    return sorted(per_bin.values(), key=lambda e: e[3]), tb.thr_index(found[best][1]) - 1


def observations(cmnd, tb):
    """Every frame of a table [F, tau_max + 1] -> (obs_v [F, N], obs_u [F], f [F, N] (0 without a candidate))."""
    F = len(cmnd)
    obs_v, obs_u, fq = np.full((F, tb.N), tb.FLOOR), np.zeros(F), np.zeros((F, tb.N))
    for k in range(F):
        cands, g = frame_candidates(cmnd[k], tb)
        obs_u[k] = tb.LU[g]
        for n, lm, f, _ in cands:
            obs_v[k, n], fq[k, n] = lm, f
    return obs_v, obs_u, fq


def _shift(x, off):
    """y[n] = x[n + off], -inf outside."""
    y = np.full_like(x, NEG_INF)
    if off >= 0:
        y[:len(x) - off] = x[off:]
    else:
        y[-off:] = x[:len(x) + off]
    return y


def viterbi(obs_v, obs_u, tb):
    """(path [F] of state indices: n voiced, N + n unvoiced; score; ties [F] bool: the winning
    predecessor of the path's state at frame k >= 1 is not alone at the maximum; final_tie: the final
    state is not)."""
    F, N, K = len(obs_u), tb.N, tb.K
    if F == 0:
        return np.zeros(0, dtype=np.int64), 0.0, np.zeros(0, dtype=bool), False
    dv, du = obs_v[0] + tb.LINIT, np.full(N, obs_u[0] + tb.LINIT)
    back = np.zeros((F, 2, N), dtype=np.int64)
    tied = np.zeros((F, 2, N), dtype=bool)
    for k in range(1, F):
        best = np.full((2, N), NEG_INF)
        for off in range(-K, K + 1):  # predecessor bin n + off, lower bins first
            pv, pu = _shift(dv, off), _shift(du, off)
            # same voicing first, then switched
            for sw, cv, cu in ((0, pv + tb.TS[abs(off)], pu + tb.TS[abs(off)]), (1, pu + tb.TX[abs(off)], pv + tb.TX[abs(off)])):
                cand = np.stack([cv, cu])
                eq = (cand == best) & (cand > NEG_INF)
                gt = cand > best
                tied[k] = np.where(gt, False, tied[k] | eq)
                back[k] = np.where(gt, (off + K) * 2 + sw, back[k])
                best = np.where(gt, cand, best)
        dv, du = obs_v[k] + best[0], obs_u[k] + best[1]
    final = np.concatenate([dv, du])
    s = int(np.argmax(final))  # the lowest index at the maximum
    score = float(final[s])
    ties = np.zeros(F, dtype=bool)
    final_tie = bool((final == final[s]).sum() > 1)
    path = np.zeros(F, dtype=np.int64)
    for k in range(F - 1, -1, -1):
        path[k] = s
        if k == 0:
            break
        voiced, n = s < N, s % N
        code = int(back[k, 0 if voiced else 1, n])
        if tied[k, 0 if voiced else 1, n]:
            ties[k] = True
        off, sw = code // 2 - K, code % 2
        s = (n + off) + (0 if voiced != bool(sw) else N)
    return path, score, ties, final_tie


def track_table(cmnd, tb):
    """A table [F, tau_max + 1] -> (f0 float64 [F], state int32 [F], score, path, ties, final_tie)."""
    obs_v, obs_u, fq = observations(cmnd, tb)
    path, score, ties, final_tie = viterbi(obs_v, obs_u, tb)
    F = len(cmnd)
    f0, state = np.zeros(F), np.full(F, -1, dtype=np.int32)
    for k, s in enumerate(path):
        if s < tb.N and fq[k, s] > 0:  # a voiced state without a candidate is reported unvoiced
            f0[k], state[k] = fq[k, s], s
    return f0, state, score, path, ties, final_tie


def track(x, tb, hop=Y.HOP, W=Y.WIN):
    """One waveform -> track_table of its own dp table."""
    return track_table(Y.table(x, hop, W, tb.tau_max)[1], tb)


def fragile(cmnd, tb, W=Y.WIN):
    """The comparisons of the candidate stage that could go the other way when every dp entry moves
    by the bound of include/fs2hip_f0.h, as tests/_f0.py: fragile: (frame, lhs, rhs) triples. The
    Viterbi stage compares sums of table values that the candidate stage's decisions select: it
    cannot change while they do not."""
    tol = 2.0 * Y.dp_ulps(W, tb.tau_max) * Y.U
    bad = []
    for k, row in enumerate(cmnd):
        tr = []
        frame_candidates(row, tb, trace=tr)
        for lhs, rhs, scale, kind in tr:
            if kind == "dp" and lhs == rhs and lhs == 1.0:
                continue  # dp == 1 exactly where cum == 0 (silence): set, not computed
            if not abs(lhs - rhs) > (1e-9 if kind == "range" else tol) * scale:  # a NaN counts as fragile
                bad.append((k, float(lhs), float(rhs)))
    return bad


# ------------------------------------------------------------------------------------------------
# what the fixture has to show (the generator refuses to write one that does not; the host test asserts it)

STEADY = ("tone75", "tone100", "tone163.7", "tone220", "tone440", "tone780")
MARGIN = Y.WIN // Y.HOP  # frames within it of an utterance edge are not "interior"
SEMITONE = 0.06


def wrong(f0, truth):
    """Frames that are dropped or more than a semitone off the truth (an octave error is 12 of them)."""
    f0, truth = np.asarray(f0), np.asarray(truth)
    return (f0 == 0) | (np.abs(f0 / truth - 1) > SEMITONE)


def voiced_ties(path, ties, final_tie, tb):
    """The ties that count against a fixture: a frame whose predecessor on the path is a voiced state
    and not alone at the maximum, or a voiced final state that is not. The N unvoiced states of a
    frame share one observation, so the routes through an unvoiced stretch that take the same steps
    in another order tie by construction (and so do the final states of an unvoiced ending); the
    stated order decides those, and tie_case tests that order."""
    path, ties = np.asarray(path), np.asarray(ties)
    bad = [int(k) for k in np.flatnonzero(ties) if path[k - 1] < tb.N]
    if final_tie and len(path) and path[-1] < tb.N:
        bad.append(len(path) - 1)
    return bad


def fixture_faults(z, verbose=False):
    """The conditions of tests/test_f0_track_host.py that fixture z misses, as a list of sentences."""
    tb = tables()
    faults = []
    say = print if verbose else (lambda *a: None)
    names = list(z["names16"])
    limits = dict({n: 2e-3 for n in STEADY}, glide120_200=1.5e-2, missing_fundamental=2e-3)
    for b, name in enumerate(names):
        n = int(z["lens16"][b])
        F = Y.n_frames(n, Y.HOP)
        x = z["wav16"][b, :n]
        dp = Y.table(x, Y.HOP, Y.WIN, tb.tau_max)[1]
        f0, state, score, path, ties, final_tie = track_table(dp, tb)
        if voiced_ties(path, ties, final_tie, tb):
            faults.append(f"{name}: the path ties at frames {np.flatnonzero(ties).tolist()} (final: {final_tie})")
        sl = slice(MARGIN, F - MARGIN)
        truth = z["truth16"][b, :F]
        if name in limits:
            if 2 * MARGIN > F // 4:
                faults.append(f"{name}: the interior leaves out {2 * MARGIN} of {F} frames")
            err = np.abs(f0[sl] / truth[sl] - 1)
            say(f"{name}: interior relative error {err.max():.3e} (limit {limits[name]})")
            if not ((f0[sl] > 0).all() and err.max() <= limits[name]):
                faults.append(f"{name}: interior error {err.max()} or an unvoiced interior frame")
        if name in ("noise", "silence", "silence_0") and (f0 > 0).any():
            faults.append(f"{name}: voiced frames {np.flatnonzero(f0 > 0).tolist()}")
        if name in ("trap", "weak"):
            yin = Y.contour_of_table(dp)[0]
            bad_y, bad_t = wrong(yin[sl], truth[sl]), wrong(f0[sl], truth[sl])
            say(f"{name}: plain YIN misses {int(bad_y.sum())} of {len(bad_y)} interior frames "
                f"({int((yin[sl] == 0).sum())} dropped), the path {int(bad_t.sum())}")
            if not bad_y.any() or bad_t.any() or 2 * MARGIN > F // 4:
                faults.append(f"{name}: plain YIN misses {int(bad_y.sum())} interior frames, the path {int(bad_t.sum())}")
    for b in range(len(z["lens200"])):
        _, _, _, path, ties, final_tie = track(z["wav200"][b, :z["lens200"][b]], tb, 200, 800)
        if voiced_ties(path, ties, final_tie, tb):
            faults.append(f"hop 200 case {b}: the path ties")
    w = z["wav32"][1, :z["lens32"][1]]
    bad = fragile(Y.table(w, Y.HOP, Y.WIN, tb.tau_max)[1], tb)
    if bad:
        faults.append(f"the general float32 case has fragile comparisons: {bad[:5]}")
    return faults


# ------------------------------------------------------------------------------------------------
# the tie order: a hand-built table over tables of small integers, whose sums are exact

TIE_PARAMS = dict(sr=1000.0, f0_floor=50.0, f0_ceil=250.0, bins_per_semitone=1, max_step=3)  # lags 4 .. 20, N = 28
TIE_TROUGHS = ({8: 0.30, 10: 0.20, 13: 0.10}, {8: 0.30, 10: 0.20, 13: 0.10}, {8: 0.30, 10: 0.20}, {10: 0.20, 13: 0.10},
               {8: 0.30, 10: 0.20, 13: 0.10})


def tie_overrides(n_bins, max_step):
    """Integer-valued tables: every candidate with a mass weighs 0, every step inside the band costs
    0, a change of voicing costs 1: all chains of candidates within reach of each other tie."""
    n1 = N_THR + 1
    lm0, lm1 = np.full((n1, n1), NEG_INF), np.full((n1, n1), NEG_INF)
    for u in range(n1):
        lm0[u, u + 1:] = 0.0
        lm1[u, u if u > 0 else 1:] = 0.0
    return dict(lm0=lm0, lm1=lm1, lu=np.full(n1 + 1, -2.0), trans_same=np.zeros(max_step + 1),
                trans_switch=np.full(max_step + 1, -1.0), log_floor=-8.0, log_init=-1.0)


def tie_case():
    """(tb, cmnd [F, 21]): the restatement's tables with the integer overrides, and dp rows that are 1
    but for the troughs of TIE_TROUGHS (equal neighbours: the parabola leaves p = t)."""
    import copy

    tb = copy.copy(tables(**TIE_PARAMS))
    o = tie_overrides(tb.N, tb.K)
    tb.LM0, tb.LM1, tb.LU, tb.TS, tb.TX = o["lm0"], o["lm1"], o["lu"], o["trans_same"], o["trans_switch"]
    tb.FLOOR, tb.LINIT = o["log_floor"], o["log_init"]
    cmnd = np.ones((len(TIE_TROUGHS), tb.tau_max + 1))
    for k, tr in enumerate(TIE_TROUGHS):
        for t, d in tr.items():
            cmnd[k, t] = d
    return tb, cmnd
