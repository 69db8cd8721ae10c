"""The host tables of the F0 tracker (include/fs2hip_f0_track.h): every logarithm, power and division
of the model, taken once per parameter set so that the device only compares, adds and looks up.

The masses are exact rationals (``fractions``) and each table entry is the double nearest its exact
value (``decimal`` at 60 digits), so that the tables, and with them the tracker's output, are the
same bits on any host: a platform's libm is not involved.
"""
import decimal
import math
from fractions import Fraction

import numpy as np
import torch

N_THR = 100  # FS2_F0_TRACK_THR
BETA_A, BETA_B = 2, 18  # the prior over thresholds: mean 0.1
P_ABSENT = Fraction(1, 100)  # p_a: what the thresholds below every candidate give to the best one
P_FLOOR = Fraction(1, 10 ** 12)
_CTX = decimal.Context(prec=60)


def _dec(q):
    q = Fraction(q)
    return _CTX.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))


def _log(q):
    """The double nearest ln(q) of an exact rational q >= 0 (-inf for 0)."""
    return float(_CTX.ln(_dec(q))) if q > 0 else float("-inf")


def n_bins(f0_floor, f0_ceil, bins_per_semitone):
    """The smallest N with f0_floor * 2^(N / (12 R)) >= f0_ceil."""
    lo, hi, R = Fraction(float(f0_floor)), Fraction(float(f0_ceil)), int(bins_per_semitone)
    if not (0 < lo < hi) or R < 1:
        raise ValueError(f"fs2amd: the tracker needs 0 < f0_floor < f0_ceil and bins_per_semitone >= 1, got "
                         f"{f0_floor}, {f0_ceil}, {bins_per_semitone}")
    n = max(int(math.ceil(12 * R * math.log2(hi / lo))) - 2, 1)
    while Fraction(2) ** n < (hi / lo) ** (12 * R):  # exact: 2^n >= (hi / lo)^(12 R)
        n += 1
    return n


class F0TrackTables:
    """thr [101], lm0 / lm1 [101, 101], lu [102], edges [N + 1], trans_same / trans_switch [K + 1] as
    float64 numpy arrays, log_floor, log_init, n_bins, max_step; ``to(device)`` uploads them once."""

    def __init__(self, sampling_rate, f0_floor, f0_ceil, bins_per_semitone=5, max_step=12, switch_prob=0.01):
        sr, R, K = float(sampling_rate), int(bins_per_semitone), int(max_step)
        sw = Fraction(float(switch_prob))
        if not sr > 0 or K < 0 or not 0 < sw < 1:
            raise ValueError(f"fs2amd: the tracker needs sampling_rate > 0, max_step >= 0 and 0 < switch_prob < 1, got "
                             f"{sampling_rate}, {max_step}, {switch_prob}")
        self.n_bins = N = n_bins(f0_floor, f0_ceil, R)
        self.max_step = K
        self.thr = np.array([i / N_THR for i in range(N_THR + 1)], dtype=np.float64)
        w = [Fraction(i, N_THR) ** (BETA_A - 1) * (1 - Fraction(i, N_THR)) ** (BETA_B - 1) for i in range(1, N_THR + 1)]
        z = sum(w)
        C = [Fraction(0)]
        for x in w:
            C.append(C[-1] + x / z)
        self.log_floor = _log(P_FLOOR)
        self.log_init = _log(Fraction(1, 2 * N))
        n1 = N_THR + 1
        self.lm0 = np.full((n1, n1), -np.inf)
        self.lm1 = np.full((n1, n1), -np.inf)
        for u in range(n1):
            for v in range(u, n1):
                own = C[v] - C[u]
                if own > 0:
                    self.lm0[u, v] = max(_log(own), self.log_floor)
                if own + P_ABSENT * C[u] > 0:
                    self.lm1[u, v] = max(_log(own + P_ABSENT * C[u]), self.log_floor)
        self.lu = np.array([_log(max((1 - P_ABSENT) * C[g] / N, P_FLOOR)) for g in range(n1)] + [_log(Fraction(1, N))])
        tri = [Fraction(K + 1 - d, (K + 1) ** 2) for d in range(K + 1)]
        self.trans_same = np.array([_log(t * (1 - sw)) for t in tri])
        self.trans_switch = np.array([_log(t * sw) for t in tri])
        two, den = decimal.Decimal(2), decimal.Decimal(12 * R)
        self.edges = np.array([float(_CTX.divide(decimal.Decimal(sr), _CTX.multiply(
            decimal.Decimal(float(f0_floor)), _CTX.power(two, _CTX.divide(decimal.Decimal(n), den))))) for n in range(N + 1)])
        self._dev = {}

    NAMES = ("thr", "lm0", "lm1", "lu", "edges", "trans_same", "trans_switch")

    def to(self, device):
        """The seven tables as contiguous float64 tensors on ``device`` (uploaded once per device)."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(getattr(self, n), dtype=np.float64)).to(device)
                                   for n in self.NAMES)
        return self._dev[key]


_TABLES = {}


def f0_track_tables(sampling_rate, f0_floor, f0_ceil, bins_per_semitone=5, max_step=12, switch_prob=0.01):
    """The cached F0TrackTables of one parameter set."""
    key = (float(sampling_rate), float(f0_floor), float(f0_ceil), int(bins_per_semitone), int(max_step), float(switch_prob))
    if key not in _TABLES:
        _TABLES[key] = F0TrackTables(*key)
    return _TABLES[key]
