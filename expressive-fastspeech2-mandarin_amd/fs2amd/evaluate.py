"""Objective evaluation on the GPU (include/fs2hip_eval.h): mel-cepstral distortion, F0 error and
voicing error along a dynamic-time-warping path, and ``evaluate``, the counterpart of the reference's
evaluate.py:18-55 (validation losses) with the MCD of a free-running synthesis beside them.

The cepstra here are DCT-II coefficients 1 .. n_coef of the model's own natural-log magnitude mel
frames, not WORLD mel-cepstra: the MCD is comparable between checkpoints of this project only.
"""
import collections
import math

import numpy as np
import torch

from .loss import FastSpeech2Loss

ALPHA = 6.141851463713754  # 10 / ln 10 * sqrt 2
LOSS_NAMES = ("total_loss", "mel_loss", "postnet_mel_loss", "pitch_loss", "energy_loss", "duration_loss")

F0Metrics = collections.namedtuple(
    "F0Metrics", "rmse_hz rmse_cents vde counts pooled_rmse_hz pooled_rmse_cents pooled_vde")
_BASIS = {}


def dct_basis(n_mel, n_coef=13):
    """Rows 1 .. n_coef of the orthonormal DCT-II of length n_mel, float64 [n_coef, n_mel]:
    sqrt(2 / n_mel) cos(pi / n_mel (m + 1/2) q). c0 (the frame's mean level) is left out."""
    if n_mel < 1 or n_coef < 1 or n_coef >= n_mel:
        raise ValueError(f"fs2amd: dct_basis needs 1 <= n_coef < n_mel, got n_coef {n_coef}, n_mel {n_mel}")
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    q = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    return np.sqrt(2.0 / n_mel) * np.cos(np.pi / n_mel * (m + 0.5) * q)


def _basis_on(device, n_mel, n_coef):
    key = (str(device), n_mel, n_coef)
    if key not in _BASIS:
        _BASIS[key] = torch.from_numpy(dct_basis(n_mel, n_coef)).to(device)
    return _BASIS[key]


def mel_cepstrum(mels, lens=None, n_coef=13):
    """Log-mel frames [B, T_max, n_mel] (float32 or float64) -> cepstra float64 [B, T_max, n_coef], zeros
    past every utterance's length (``ops.mel_cepstrum`` with the table of ``dct_basis``)."""
    from . import ops

    ops._gpu(mels)
    return ops.mel_cepstrum(mels, lens, basis=_basis_on(mels.device, mels.shape[-1], n_coef))


def dtw(x, x_lens, y, y_lens, bitmap="auto"):
    """``ops.dtw``: the warping path of x [B, Tx_max, D] onto y [B, Ty_max, D] under the Euclidean
    frame distance -> ops.DtwOut(total, K, path_i, path_j), the alignment ``f0_metrics`` takes."""
    from . import ops

    return ops.dtw(x, x_lens, y, y_lens, bitmap=bitmap)


def mcd(mels_a, lens_a, mels_b, lens_b, n_coef=13):
    """Mel-cepstral distortion in dB per utterance, float64 [B]: ALPHA * total_b / K_b over the DTW
    path between the cepstra of the two log-mel batches, and the alignment it was read along."""
    from . import ops

    ca = mel_cepstrum(mels_a, lens_a, n_coef)
    cb = mel_cepstrum(mels_b, lens_b, n_coef)
    al = ops.dtw(ca, lens_a, cb, lens_b)
    return ALPHA * al.total / al.K.to(torch.float64), al


def f0_metrics(f0_a, f0_b, alignment):
    """F0 contours in Hz [B, Tx_max] and [B, Ty_max] (0 = unvoiced) along ``alignment`` -> F0Metrics:
    per utterance the RMSE in Hz and in cents over the pairs voiced on both sides (NaN where there is
    none), the voicing-decision error (pairs voiced on one side only) / K, the counts int64 [B, 4] =
    both, a only, b only, neither; and the three figures pooled over the batch."""
    from . import ops

    ops._gpu(f0_a, f0_b)
    if f0_a.dim() != 2 or f0_b.dim() != 2 or f0_a.shape[0] != f0_b.shape[0]:
        raise ValueError("fs2amd: f0_metrics takes f0_a [B, Tx_max] and f0_b [B, Ty_max]")

    def tracks(f0):
        f0 = f0.to(torch.float64)
        nan = torch.full_like(f0, float("nan"))
        voiced = f0 > 0
        hz = torch.where(voiced, f0, nan)
        return torch.stack((hz, 1200.0 * torch.log2(hz)), dim=-1).contiguous()

    st = ops.path_stats(tracks(f0_a), tracks(f0_b), alignment.path_i, alignment.path_j, alignment.K)
    n_both = st.counts[:, :, 0].to(torch.float64)
    rmse = torch.sqrt(st.sums[:, :, 1] / n_both)
    counts = st.counts[:, 0, :]
    K = alignment.K.to(torch.float64)
    wrong = (counts[:, 1] + counts[:, 2]).to(torch.float64)
    pooled = torch.sqrt(st.sums[:, :, 1].sum(0) / n_both.sum(0))
    return F0Metrics(rmse[:, 0], rmse[:, 1], wrong / K, counts, pooled[0], pooled[1], wrong.sum() / K.sum())


def evaluate(model, batches, preprocess_config, model_config, n_coef=13):
    """The reference's evaluate.py:18-55 over ``batches`` (device tuples as ``pipeline.to_device``
    gives them): the six FastSpeech2Loss means of the teacher-forced forward, weighted by batch size,
    and the mean MCD of a free-running synthesis (no targets passed) against the ground-truth mels.
    Returns a dict: LOSS_NAMES -> float, "mcd" (mean over the utterances the model gave at least one
    frame; NaN if none), "n_utts", "n_mcd". The model's mode and parameters are left as found."""
    loss_fn = FastSpeech2Loss(preprocess_config, model_config)
    was_training = model.training
    model.eval()
    sums, n_utts, mcd_sum, n_mcd = None, 0, None, None
    try:
        with torch.no_grad():
            for batch in batches:
                n = len(batch[0])
                losses = loss_fn(batch, model(*batch[2:]))
                part = torch.stack([l.detach().to(torch.float64) for l in losses]) * n
                sums = part if sums is None else sums + part
                n_utts += n
                syn = model(*batch[2:9])
                mel_syn, syn_lens = syn[1].float(), syn[9]
                if mel_syn.shape[1] < 1:
                    continue
                m, _ = mcd(mel_syn, syn_lens, batch[9].float(), batch[10], n_coef)
                ok = torch.isfinite(m)
                s, c = torch.where(ok, m, torch.zeros_like(m)).sum(), ok.sum()
                mcd_sum, n_mcd = (s, c) if mcd_sum is None else (mcd_sum + s, n_mcd + c)
    finally:
        model.train(was_training)
    if n_utts == 0:
        raise ValueError("fs2amd: evaluate got no batches")
    out = dict(zip(LOSS_NAMES, (sums / n_utts).tolist()))
    n_mcd = 0 if n_mcd is None else int(n_mcd)
    out.update(mcd=float(mcd_sum) / n_mcd if n_mcd else math.nan, n_utts=n_utts, n_mcd=n_mcd)
    return out
