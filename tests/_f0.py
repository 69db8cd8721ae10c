"""The F0 estimator of include/fs2hip_f0.h restated in plain numpy, operation for operation: the
oracle of the F0 tests (the reference's estimator, pyworld, is not installed anywhere this suite
runs, and this estimator is YIN, not WORLD's: there is nothing of the reference's to compare with).

``table`` builds d -> cum -> dp per frame with the sum of d in one of three orders (the contract
leaves it free; on int16 input all three are the same bits), ``pick`` goes from one dp row to
(f0, tau) and takes any table, the GPU's own included, ``fragile`` lists the comparisons of a pick
that rounding could flip. numpy has no fused multiply-add: the square of a term is rounded before
it is added, which the header's error bound covers.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR, HOP, WIN, F0_FLOOR, F0_CEIL, THR = 22050.0, 256, 1024, 71.0, 800.0, 0.1
U = 2.0 ** -53


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "f0_a.npz")))


def ragged(z, key, lens_key):
    return [z[key][i, :n] for i, n in enumerate(z[lens_key])]


def lags(sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    return int(math.floor(sr / f0_ceil)), int(math.ceil(sr / f0_floor))


def dp_ulps(W, tau):
    """FS2_F0_DP_ULPS of the header."""
    return 2 * W + tau + 6


def n_frames(n, hop):
    return n // hop + 1


def table(x, hop=HOP, W=WIN, tau_max=None, order="forward"):
    """(d, dp), both float64 [F, tau_max + 1], of samples x (int16 or float32, converted to double).
    order: "forward" / "backward" over j, or "blocks": hop-sized blocks of j summed forward each,
    then added left to right, then the tail W % hop (the kernel's order)."""
    tau_max = lags()[1] if tau_max is None else tau_max
    x = np.asarray(x).astype(np.float64)
    n = len(x)
    F = n_frames(n, hop)
    off = (W + tau_max) // 2
    xp = np.zeros(off + (F - 1) * hop + W + tau_max + 1)
    xp[off:off + n] = x
    base = np.arange(F) * hop  # frame k starts at k * hop - off, which is xp[k * hop]
    taus = np.arange(1, tau_max + 1)

    def run(js):
        acc = np.zeros((F, tau_max))
        for j in js:
            diff = xp[base + j][:, None] - xp[(base + j)[:, None] + taus[None, :]]
            acc = acc + diff * diff
        return acc

    if order == "forward":
        d1 = run(range(W))
    elif order == "backward":
        d1 = run(range(W - 1, -1, -1))
    else:
        q = W // hop
        d1 = np.zeros((F, tau_max))
        for m in range(q):
            d1 = d1 + run(range(m * hop, (m + 1) * hop))
        if W % hop:
            d1 = d1 + run(range(q * hop, W))
    d = np.zeros((F, tau_max + 1))
    d[:, 1:] = d1
    cum = np.zeros((F, tau_max + 1))
    for t in range(1, tau_max + 1):  # left to right
        cum[:, t] = cum[:, t - 1] + d[:, t]
    dp = np.ones((F, tau_max + 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        val = (d * np.arange(tau_max + 1, dtype=np.float64)[None, :]) / cum
    nz = ~(cum == 0.0)
    nz[:, 0] = False
    dp[nz] = val[nz]
    return d, dp


def pick(dp, sr=SR, tau_min=None, tau_max=None, thr=THR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, trace=None):
    """One dp row [tau_max + 1] -> (f0, tau). trace: a list that receives every comparison made as
    (lhs, rhs, scale, kind) with scale the magnitude the gap is relative to and kind "dp" (between
    table entries, or one and a constant) or "range" (f against a limit)."""
    if tau_min is None:
        tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    dp = np.asarray(dp, dtype=np.float64)
    note = trace.append if trace is not None else (lambda c: None)
    t = None
    for c in range(tau_min, tau_max):
        note((dp[c], thr, max(abs(dp[c]), thr), "dp"))
        if dp[c] < thr:
            t = c
            break
    if t is None:
        return 0.0, 0
    while t + 1 < tau_max:
        note((dp[t + 1], dp[t], max(abs(dp[t + 1]), abs(dp[t])), "dp"))
        if not dp[t + 1] < dp[t]:
            break
        t += 1
    a, b, c = dp[t - 1], dp[t], dp[t + 1]
    den = (a - np.float64(2.0) * b) + c
    note((den, 0.0, abs(a) + 2 * abs(b) + abs(c), "dp"))
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = (np.float64(0.5) * (a - c)) / den if den > 0 else np.float64(0.0)
        f = np.float64(sr) / (np.float64(t) + delta)
    note((f, f0_floor, f0_floor, "range"))
    note((f, f0_ceil, f0_ceil, "range"))
    if f0_floor <= f <= f0_ceil:
        return float(f), t
    return 0.0, 0


def contour(x, sr=SR, hop=HOP, W=WIN, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, thr=THR, order="forward"):
    """(f0 float64 [F], tau int32 [F], dp [F, tau_max + 1]) of one waveform."""
    tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    _, dp = table(x, hop, W, tau_max, order)
    return contour_of_table(dp, sr, f0_floor, f0_ceil, thr) + (dp,)


def contour_of_table(dp, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, thr=THR):
    tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    res = [pick(row, sr, tau_min, tau_max, thr, f0_floor, f0_ceil) for row in dp]
    return (np.array([r[0] for r in res], dtype=np.float64).reshape(len(dp)),
            np.array([r[1] for r in res], dtype=np.int32).reshape(len(dp)))


def fragile(dp, W=WIN, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, thr=THR):
    """The frames of a table in which a comparison of the pick could go the other way under the
    header's bound: a gap between two dp values (each off by the bound at most) or between dp and the
    threshold below twice FS2_F0_DP_ULPS * 2^-53 of the larger side, a denominator that close to 0
    relative to its terms, or an f within 1e-9 (relative) of a range limit. Returns (frame, lhs,
    rhs) triples."""
    tau_min, tau_max = lags(sr, f0_floor, f0_ceil)
    tol = 2.0 * dp_ulps(W, tau_max) * U
    bad = []
    for k, row in enumerate(dp):
        tr = []
        pick(row, sr, tau_min, tau_max, thr, f0_floor, f0_ceil, trace=tr)
        for lhs, rhs, scale, kind in tr:
            if not abs(lhs - rhs) > (tol if kind == "dp" else 1e-9) * scale:  # a NaN counts as fragile
                bad.append((k, float(lhs), float(rhs)))
    return bad
