"""Float64 numpy restatement of the conditioning with weights over the embedding rows (what the
model computes when every nn.Embedding(ids) is replaced by weights @ table):

    e = w_e . E,  a = w_a . A,  v = w_v . V;   emo = relu(W . cat(e, a, v) + b);   spk = w_s . S

Each input is ids [B] (a one-hot row), weights [B, n], or (emotions / arousals / valences) weights
[B, L, n]; with a curve among the three the others broadcast over L. Weights are used as given.
The vectors are added at every position i < L, padded ones included."""
import numpy as np


def weight_rows(t, n):
    """ids [B] -> one-hot f64 [B, n]; weights [B, n] / [B, L, n] -> f64, unchanged."""
    t = np.asarray(t)
    if np.issubdtype(t.dtype, np.integer):
        assert t.ndim == 1 and t.min() >= 0 and t.max() < n
        return np.eye(n, dtype=np.float64)[t]
    assert t.ndim in (2, 3) and t.shape[-1] == n, t.shape
    return t.astype(np.float64)


def speaker_vectors(spk_table, speakers):
    """(spk f64 [B, D], S f64 [B, D] = sum_j |w_j| |table[j]|: the scale of the rounding bound)."""
    T = np.asarray(spk_table, np.float64)
    w = weight_rows(speakers, T.shape[0])
    assert w.ndim == 2
    return w @ T, np.abs(w) @ np.abs(T)


def emotion_vectors(P, emotions, arousals, valences, L=None):
    """(emo, S): emo f64 [B, D], or [B, L, D] when an input is a curve (or L is given);
    S = sum_k |W[n, k]| |cat[k]| + |b[n]| of the same shape. P: emo_table, aro_table, val_table,
    lin_w, lin_b."""
    tabs = [np.asarray(P[k], np.float64) for k in ("emo_table", "aro_table", "val_table")]
    ws = [weight_rows(t, T.shape[0]) for t, T in zip((emotions, arousals, valences), tabs)]
    if L is None and any(w.ndim == 3 for w in ws):
        L = next(w.shape[1] for w in ws if w.ndim == 3)
    if L is not None:
        ws = [w if w.ndim == 3 else np.repeat(w[:, None, :], L, axis=1) for w in ws]
        assert all(w.shape[1] == L for w in ws)
    cat = np.concatenate([w @ T for w, T in zip(ws, tabs)], axis=-1)
    W, b = np.asarray(P["lin_w"], np.float64), np.asarray(P["lin_b"], np.float64)
    return np.maximum(cat @ W.T + b, 0.0), np.abs(cat) @ np.abs(W).T + np.abs(b)


def add(x, spk=None, emo=None):
    """x [B, L, D] + spk [B, D] + emo [B, D] or [B, L, D], at every position, in float64."""
    y = np.asarray(x, np.float64).copy()
    if spk is not None:
        y = y + spk[:, None, :]
    if emo is not None:
        y = y + (emo if emo.ndim == 3 else emo[:, None, :])
    return y
