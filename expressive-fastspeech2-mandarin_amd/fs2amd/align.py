"""Durations without a forced aligner: the alignment-learning framework of Badlani et al. 2021
("One TTS Alignment To Rule Them All") on the kernels of include/fs2hip_align.h.

* ``AlignmentEncoder`` — a small network (plain torch) that scores every (mel frame, phoneme) pair.
* ``ForwardSumLoss`` — trains it: the CTC likelihood of "phonemes 1..L in order" (``ops.forward_sum`` and
  ``ops.forward_sum_bwd``, float64 on the GPU, one launch over the ragged batch each).
* ``mas_durations`` — monotonic alignment search (``ops.mas``): the soft map to hard durations.
* ``beta_binomial_prior`` — the usual diagonal prior (host code on scipy).
* ``fit_aligner`` / ``align`` / ``Aligner`` — the training loop, the inference call, and the object
  ``fs2amd.build_corpus(aligner=...)`` takes.

The reference has none of this: it reads durations from MFA TextGrids. Using the aligner inside the
FastSpeech2 training step is not part of it either.
"""
import functools

import numpy as np
import torch
from torch import nn


class _ForwardSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, mel_lens, text_lens, blank_logprob):
        from . import ops

        if logp.dim() == 3 and logp.shape[2] > 1 and logp.stride(2) != 1:
            logp = logp.contiguous()
        logp = logp.detach()
        o = ops.forward_sum(logp, mel_lens, text_lens, blank_logprob=blank_logprob)
        ctx.save_for_backward(logp, o.alpha, o.nll)
        ctx.lens, ctx.blank_logprob = (mel_lens, text_lens), blank_logprob
        return o.loss

    @staticmethod
    def backward(ctx, grad_out):
        from . import ops

        logp, alpha, nll = ctx.saved_tensors
        grad = ops.forward_sum_bwd(logp, ctx.lens[0], ctx.lens[1], alpha, nll, grad_out,
                                   blank_logprob=ctx.blank_logprob)
        return grad, None, None, None


class ForwardSumLoss(nn.Module):
    """``loss = crit(attn_logprob, mel_lens, text_lens)``: attn_logprob f32 or f64 [B, T_max, L_max] on
    the GPU, the lengths as tensors (host or device) or lists. The mean over the batch of the CTC
    negative log-likelihood per phoneme, a float64 scalar; an utterance with fewer frames than
    phonemes contributes 0 (zero_infinity). The gradient is exactly 0 outside every [T_b, L_b]."""

    def __init__(self, blank_logprob=-1.0):
        super().__init__()
        self.blank_logprob = float(blank_logprob)

    def forward(self, attn_logprob, mel_lens, text_lens):
        return _ForwardSumFn.apply(attn_logprob, mel_lens, text_lens, self.blank_logprob)


def mas_durations(attn_logprob, mel_lens, text_lens):
    """Hard durations from a soft alignment: a list with an int64 numpy array [L_b] per utterance,
    every entry >= 1, summing to T_b. Lengths as ``ops.mas`` takes them; host lengths are checked
    (T_b >= L_b >= 1)."""
    from . import ops

    text = torch.as_tensor(text_lens).cpu().tolist()
    dur = ops.mas(attn_logprob.detach(), mel_lens, text_lens).durations.cpu().numpy()
    return [dur[b, :int(n)].copy() for b, n in enumerate(text)]


@functools.lru_cache(maxsize=4096)
def _prior_cached(L, T, scaling):
    from scipy.stats import betabinom

    k = np.arange(L)
    t = np.arange(1, T + 1, dtype=np.float64)[:, None]
    return betabinom.pmf(k[None, :], L - 1, scaling * t, scaling * (T + 1 - t))


def beta_binomial_prior(L, T, scaling=1.0):
    """The diagonal prior, float64 [T, L]: row t is the pmf of BetaBinomial(L - 1, scaling * (t + 1),
    scaling * (T - t)) over the phonemes 0 .. L - 1; every row sums to 1."""
    L, T = int(L), int(T)
    if L < 1 or T < 1:
        raise ValueError(f"fs2amd: beta_binomial_prior needs L, T >= 1, got {L}, {T}")
    return _prior_cached(L, T, float(scaling)).copy()


class AlignmentEncoder(nn.Module):
    """Scores every (mel frame, phoneme) pair: ``attn_logprob = enc(phone_ids, text_lens, mels, mel_lens)``
    with phone_ids int64 [B, L_max], mels float32 [B, T_max, n_mel], the lengths on the host ->
    float32 [B, T_max, L_max]:

        log_softmax_j(-temperature * |q_t - k_j|^2) + log(prior[t, j] + 1e-8),   -inf for j >= L_b

    keys from an own phoneme embedding (Conv1d k=3, ReLU, Conv1d k=1 down to d_att), queries from the
    mel (Conv1d k=3, ReLU, Conv1d k=1, ReLU, Conv1d k=1). The distance is |q|^2 + |k|^2 - 2 q.k with
    one bmm; the [B, C, T, L] difference is never formed. prior: True = ``beta_binomial_prior`` of
    every utterance's own (L_b, T_b)."""

    def __init__(self, n_symbols, n_mel=80, d_text=256, d_att=80, temperature=0.0005, prior=True, prior_scaling=1.0):
        super().__init__()
        self.temperature, self.prior, self.prior_scaling = float(temperature), bool(prior), float(prior_scaling)
        self.embedding = nn.Embedding(n_symbols, d_text)
        self.key_proj = nn.Sequential(nn.Conv1d(d_text, 2 * d_text, 3, padding=1), nn.ReLU(),
                                      nn.Conv1d(2 * d_text, d_att, 1))
        self.query_proj = nn.Sequential(nn.Conv1d(n_mel, 2 * n_mel, 3, padding=1), nn.ReLU(),
                                        nn.Conv1d(2 * n_mel, n_mel, 1), nn.ReLU(), nn.Conv1d(n_mel, d_att, 1))

    def log_prior(self, text_lens, mel_lens, T_max, L_max, device):
        out = np.zeros((len(text_lens), T_max, L_max), dtype=np.float32)
        for b, (n, t) in enumerate(zip(text_lens, mel_lens)):
            if n >= 1 and t >= 1:
                out[b, :t, :n] = np.log(beta_binomial_prior(n, t, self.prior_scaling) + 1e-8)
        return torch.from_numpy(out).to(device)

    def forward(self, phone_ids, text_lens, mels, mel_lens):
        text_lens = [int(v) for v in torch.as_tensor(text_lens).cpu().tolist()]
        mel_lens = [int(v) for v in torch.as_tensor(mel_lens).cpu().tolist()]
        B, L_max = phone_ids.shape
        T_max = mels.shape[1]
        dev = mels.device
        tmask = torch.arange(L_max, device=dev)[None, :] >= torch.tensor(text_lens, device=dev)[:, None]  # [B, L]
        mmask = torch.arange(T_max, device=dev)[None, :] >= torch.tensor(mel_lens, device=dev)[:, None]   # [B, T]
        emb = self.embedding(phone_ids).masked_fill(tmask[:, :, None], 0.0)
        k = self.key_proj(emb.transpose(1, 2))                                                  # [B, C, L]
        q = self.query_proj(mels.masked_fill(mmask[:, :, None], 0.0).transpose(1, 2)).transpose(1, 2)  # [B, T, C]
        dist = (q * q).sum(2)[:, :, None] + (k * k).sum(1)[:, None, :] - 2.0 * torch.bmm(q, k)  # [B, T, L]
        score = (-self.temperature * dist).masked_fill(tmask[:, None, :], float("-inf"))
        logp = torch.log_softmax(score, dim=2)
        if self.prior:
            logp = logp + self.log_prior(text_lens, mel_lens, T_max, L_max, dev)
        return logp.masked_fill(tmask[:, None, :], float("-inf"))


def fit_aligner(encoder, batches, *, steps, lr=1e-3, blank_logprob=-1.0):
    """Adam on ``ForwardSumLoss``: ``batches`` yields (phone_ids, text_lens, mels, mel_lens) (tensors as
    ``AlignmentEncoder`` takes them; the iterable is walked again when it runs out) for ``steps``
    steps. Returns the loss of every step as a list of floats."""
    crit = ForwardSumLoss(blank_logprob)
    opt = torch.optim.Adam(encoder.parameters(), lr=lr)
    encoder.train()
    history, it = [], iter(batches)
    for _ in range(int(steps)):
        try:
            batch = next(it)
        except StopIteration:
            it = iter(batches)
            batch = next(it)
        phone_ids, text_lens, mels, mel_lens = batch
        opt.zero_grad(set_to_none=True)
        loss = crit(encoder(phone_ids, text_lens, mels, mel_lens), mel_lens, text_lens)
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    return history


def align(encoder, phone_ids, text_lens, mels, mel_lens):
    """Durations of a batch as ``mas_durations`` gives them, under ``torch.no_grad()``."""
    was_training = encoder.training
    encoder.eval()
    try:
        with torch.no_grad():
            return mas_durations(encoder(phone_ids, text_lens, mels, mel_lens), mel_lens, text_lens)
    finally:
        encoder.train(was_training)


class Aligner:
    """What ``build_corpus(aligner=...)`` takes: ``symbols`` (phoneme label -> id) and
    ``durations(phone_ids_list, mels_list)`` over an ``AlignmentEncoder`` on the GPU. phone_ids_list:
    integer arrays [L_b]; mels_list: float32 arrays [T_b, n_mel]. Returns int64 arrays [L_b] that sum
    to T_b."""

    def __init__(self, encoder, symbols):
        self.encoder, self.symbols = encoder, dict(symbols)

    def pack(self, phone_ids_list, mels_list):
        dev = next(self.encoder.parameters()).device
        B = len(phone_ids_list)
        text_lens = torch.tensor([len(p) for p in phone_ids_list], dtype=torch.int64)
        mel_lens = torch.tensor([len(m) for m in mels_list], dtype=torch.int64)
        ids = torch.zeros(B, max(int(text_lens.max()), 1), dtype=torch.int64)
        n_mel = np.asarray(mels_list[0]).shape[1]
        mels = torch.zeros(B, max(int(mel_lens.max()), 1), n_mel, dtype=torch.float32)
        for b, (p, m) in enumerate(zip(phone_ids_list, mels_list)):
            ids[b, :len(p)] = torch.as_tensor(np.asarray(p), dtype=torch.int64)
            mels[b, :len(m)] = torch.as_tensor(np.asarray(m), dtype=torch.float32)
        return ids.to(dev), text_lens, mels.to(dev), mel_lens

    def fit(self, phone_ids_list, mels_list, *, steps, lr=1e-3):
        return fit_aligner(self.encoder, [self.pack(phone_ids_list, mels_list)], steps=steps, lr=lr)

    def durations(self, phone_ids_list, mels_list):
        if len(phone_ids_list) != len(mels_list):
            raise ValueError("fs2amd: one mel per phoneme sequence")
        if not phone_ids_list:
            return []
        return align(self.encoder, *self.pack(phone_ids_list, mels_list))
