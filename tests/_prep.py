"""Host restatement (numpy only) of the reference's preprocessing arithmetic, the yardstick of
test_prep_host.py and test_gpu_prep.py:

* ``pitch_target``  — preprocessor/preprocessor.py:263-291: crop to sum(duration), scipy's linear
  ``interp1d`` over the voiced frames written out operation for operation, then the in-place
  phoneme-mean loop.
* ``outlier_fence`` — :367-375 with numpy's default percentile written out in the element type.
* ``normalize``     — :377-388 over a list of arrays.
* ``exact_mean_var`` — the exact (rational) mean and population variance of a set of samples, and
  ``scaler_ratios``: an approximation's relative errors as multiples of the bound for updating
  algorithms (Chan, Golub, LeVeque 1983).

tests/golden/gen_golden_prep.py asserts that these equal the reference's own calls (scipy, numpy,
sklearn, the reference's Preprocessor methods) before it writes tests/golden/prep_a.npz.
"""
import math
import os
from fractions import Fraction

import numpy as np

from _npz_parts import load_npz_parts

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "prep_a.npz")


def load_fixture():
    return load_npz_parts(FIXTURE)


def ragged(z, key, lens_key):
    """The list of arrays stored concatenated as z[key] with lengths z[lens_key]."""
    off = np.concatenate([[0], np.cumsum(z[lens_key])])
    return [z[key][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def interp_voiced(pitch):
    """interp1d(ids, pitch[ids], fill_value=(pitch[ids[0]], pitch[ids[-1]]), bounds_error=False)(
    arange(len(pitch))) for a float64 contour with at least two non-zero frames."""
    ids = np.where(pitch != 0)[0]
    y = pitch[ids]
    t = np.arange(len(pitch))
    hi = np.searchsorted(ids, t).clip(1, len(ids) - 1)
    lo = hi - 1
    x_lo, x_hi, y_lo, y_hi = ids[lo], ids[hi], y[lo], y[hi]
    slope = (y_hi - y_lo) / (x_hi - x_lo)
    out = slope * (t - x_lo) + y_lo
    out[t < ids[0]] = y[0]
    out[t > ids[-1]] = y[-1]
    return out


def segment_mean_loop(values, duration):
    """The in-place loop of :283-291 on a copy."""
    v = np.array(values, copy=True)
    pos = 0
    for i, d in enumerate(duration):
        v[i] = np.mean(v[pos:pos + d]) if d > 0 else 0
        pos += d
    return v[:len(duration)]


def pitch_target(f0, duration):
    """(phoneme-level pitch [L], interpolated contour [n], voiced count); the first two None where
    the reference drops the utterance."""
    pitch = np.asarray(f0, dtype=np.float64)[:int(np.sum(duration))]
    voiced = int(np.sum(pitch != 0))
    if voiced <= 1:
        return None, None, voiced
    filled = interp_voiced(pitch)
    return segment_mean_loop(filled, duration), filled, voiced


def mean_bounds(filled, duration):
    """Per phoneme d_i * 2^-52 * max|segment|: the bound of a d-term float64 sum, on both sides."""
    pos = np.concatenate([[0], np.cumsum(duration)])
    return np.array([d * 2.0 ** -52 * (np.abs(filled[pos[i]:pos[i + 1]]).max() if d > 0 else 0.0)
                     for i, d in enumerate(duration)])


def quantile_linear(sorted_v, q):
    """numpy's method="linear" on a sorted array, every operation in the array's dtype."""
    E = sorted_v.dtype.type
    n = len(sorted_v)
    vi = E(q) * E(n - 1)
    fl = np.floor(vi)
    g = vi - fl
    lo = int(fl)
    hi = lo + 1
    if lo >= n - 1:
        lo = hi = n - 1
    a, b = sorted_v[lo], sorted_v[hi]
    diff = b - a
    return b - diff * (E(1) - g) if g >= E(0.5) else a + diff * g


def outlier_fence(values):
    """(mask, p25, p75) of :367-375 for a float32 or float64 array; an empty one gives NaN quartiles."""
    values = np.asarray(values)
    E = values.dtype.type
    if len(values) == 0:
        return np.zeros(0, dtype=bool), E(np.nan), E(np.nan)
    s = np.sort(values)
    with np.errstate(invalid="ignore"):
        p25, p75 = quantile_linear(s, 0.25), quantile_linear(s, 0.75)
        w = E(1.5) * (p75 - p25)
        lower, upper = p25 - w, p75 + w
    return np.logical_and(values > lower, values < upper), p25, p75


def normalize(arrays, mean, std):
    """:377-388: ((v - mean) / std per array, min, max)."""
    max_value, min_value = np.finfo(np.float64).min, np.finfo(np.float64).max
    out = []
    for v in arrays:
        values = (v - mean) / std
        out.append(values)
        max_value = max(max_value, max(values))
        min_value = min(min_value, min(values))
    return out, min_value, max_value


class ExactMoments:
    """Exact (rational) running count, sum and sum of squares of float samples."""

    def __init__(self):
        self.n, self.sx, self.sxx = 0, Fraction(0), Fraction(0)

    def add(self, samples):
        for x in samples:
            x = Fraction(float(x))
            self.sx += x
            self.sxx += x * x
        self.n += len(samples)
        return self

    def mean_var(self):
        """(mean, population variance) as Fractions."""
        mean = self.sx / self.n
        return mean, self.sxx / self.n - mean * mean

    def ratios(self, mean, var):
        """(mean ratio, variance ratio): relative errors of mean / var against the exact values,
        divided by N * 2^-53 and N * 2^-53 * kappa, kappa = sqrt(1 + mean^2 / var) (the bound for
        updating algorithms). At or below 1 is within the bound."""
        em, ev = self.mean_var()
        if ev == 0 or em == 0:  # not reached by the fixture; exactness is then the only sensible demand
            return (0.0 if Fraction(float(mean)) == em else math.inf), (0.0 if Fraction(float(var)) == ev else math.inf)
        kappa = math.sqrt(1.0 + float(em * em / ev))
        u = self.n * 2.0 ** -53
        r_mean = abs(float((Fraction(float(mean)) - em) / em)) / u
        r_var = abs(float((Fraction(float(var)) - ev) / ev)) / (u * kappa)
        return r_mean, r_var


def exact_mean_var(samples):
    """(mean, population variance) of float samples as exact Fractions."""
    return ExactMoments().add(samples).mean_var()


def scaler_ratios(mean, var, samples):
    """ExactMoments.ratios over one set of samples."""
    return ExactMoments().add(samples).ratios(mean, var)
