"""The HIP hot path as ``torch.library`` custom ops ("registered as torch.library ops
(fs2::length_regulate, ...) so autograd and DDP work").

Each op wraps the C-ABI launch of :mod:`fs2amd.ops` (no CPU fallback: CPU tensors raise, as every
entry point does) and carries a fake (meta) implementation, so ``torch.compile`` / ``torch.export``
trace through it with ``fullgraph=True`` instead of breaking the graph at a ctypes call:

* ``fs2::length_regulate(x, duration, max_len) -> (out, mel_len)`` —
  ``LengthRegulator.forward`` (model/modules.py:161-194 + utils/tools.py:360-378); ``max_len <= 0``
  means max(mel_len) (a data-dependent size: an unbacked symbol under tracing).
* ``fs2::attention(qkv, lens, n_head, d_k, temperature) -> out`` — ``ScaledDotProductAttention`` with
  the key-padding mask and the head split / merge (transformer/Modules.py:14-25,
  transformer/SubLayers.py:36-52) over the fused [B, T, 3·H·dk] projection; differentiable
  (backward: ``fs2::attention_bwd``, the flash-style recompute of fs2_attention_bwd).
* ``fs2::attention_bwd(qkv, out, dout, lens, n_head, d_k, temperature) -> dqkv`` (f32).
* ``fs2::ffn(x, w_packed, b1, b2, ln_gamma, ln_beta, ln_eps, lens, ks, pad) -> y`` — the FFT block's
  ``PositionwiseFeedForward`` + residual + LayerNorm + padding mask (transformer/SubLayers.py:85-93,
  transformer/Layers.py:28) as one fs2_ffn launch (inference; weights from ops.pack_ffn_weights).
* ``fs2::conv1d(x, w_packed, bias, cin, ks, pad, compute, epilogue, out_dtype) -> y`` — fs2_conv1d
  with a plain (bias / activation) epilogue.
* ``fs2::mel_spectrogram(wav, lens, forward_basis, mel_basis, T_out, hop, win, max_wav_value, clip_val)
  -> (mel, energy, frames)`` — ``TacotronSTFT.mel_spectrogram`` (audio/stft.py:130-178) over a ragged
  batch as one fs2_mel_spectrogram launch: mel f32 [B, T_out, n_mel] channels-last, energy f32
  [B, T_out], frames int64 [B]; ``lens`` on the device (or None: full rows), ``T_out`` a host int.
* ``fs2::stft(wav, lens, forward_basis, T_out, hop, win, clip) -> (spec, mag, frames)`` —
  ``STFT.transform``'s convolution (audio/stft.py:52-78) over a ragged batch as one fs2_stft launch: spec
  f32 [B, 1026, T_out] (re rows, then im rows), mag f32 [B, 513, T_out], frames int64 [B].
* ``fs2::istft(recomb, frames, inverse_packed, wsum_table, n_out_max, hop, win) -> (wav, lens_out)`` —
  ``STFT.inverse`` after its recombination (audio/stft.py:88-122) as one fs2_istft launch: wav f32
  [B, n_out_max], lens_out int64 [B] = hop * max(frames - 1, 0).
* ``fs2::pitch_targets(f0, dur, frames) -> (out, filled, voiced)``, ``fs2::outlier_moments(values, lens)
  -> (quartiles, inlier, count, mean, m2)``, ``fs2::moments_merge(state, count, mean, m2)`` (mutates
  ``state``) and ``fs2::normalize_minmax(values, lens, mean, std) -> (out, minmax)`` — the corpus
  preprocessing of preprocessor/preprocessor.py:263-291, :367-375, :152-155 and :377-388
  (include/fs2hip_prep.h), float64 results.
* ``fs2::f0_yin(wav, lens, sampling_rate, hop, win, f0_floor, f0_ceil, threshold) -> (f0, tau, cmnd)`` —
  the F0 contour of a ragged waveform batch (include/fs2hip_f0.h: YIN in float64, not the reference's
  pyworld call): f0 f64 [B, n_max // hop + 1], tau int32 likewise, cmnd f64 [B, n_max // hop + 1, tau_max + 1].
* ``fs2::resample(wav, lens, taps, up, down) -> (y, y32, peak, out_lens)`` and ``fs2::peak_int16(y32, peak,
  out_lens, max_wav_value) -> int16 rows`` — the reference's prepare_align arithmetic
  (preprocessor/esd_chinese.py:145-147) over a ragged batch (include/fs2hip_resample.h): y f64
  [B, ceil(n_max * up / down)] bit for bit scipy.signal.resample_poly's, y32 its f32 rounding, peak f32 [B].
* ``fs2::mas(logp, mel_lens, text_lens) -> (durations, score, path)`` — monotonic alignment search over
  attention log-probabilities [B, T_max, L_max] (include/fs2hip_align.h): durations int64 [B, L_max], score
  f64 [B], path int32 [B, T_max], bit for bit the float64 recurrence; a tie takes the diagonal.
* ``fs2::forward_sum(logp, mel_lens, text_lens, blank_logprob) -> (loss, nll, alpha)`` — the alignment
  (CTC) loss of the same header in float64: loss f64 scalar, nll f64 [B], alpha f64 [B, T_max, 2 L_max + 1];
  differentiable in ``logp`` through ``loss`` (backward: ``fs2::forward_sum_bwd``).
* ``fs2::forward_sum_bwd(logp, mel_lens, text_lens, alpha, nll, grad_out, blank_logprob) -> dlogp`` (logp's
  dtype, exact zeros outside every utterance's extents).
* ``fs2::mel_cepstrum(mel, lens, basis) -> cepstra`` — log-mel [B, T_max, M] times the f64 table basis
  [C, M] (include/fs2hip_eval.h): f64 [B, T_max, C], summed in index order, zeros past every T_b.
* ``fs2::pair_dist(x, x_lens, y, y_lens) -> cost`` — Euclidean distances between the frames of
  x [B, Tx_max, D] and y [B, Ty_max, D] in float64: f64 [B, Tx_max, Ty_max], zeros outside [Tx_b, Ty_b].
* ``fs2::f0_track(cmnd, lens, sampling_rate, hop, f0_floor, f0_ceil, bins_per_semitone, max_step, switch_prob)
  -> (f0, state, score)`` — an F0 path through the utterance over the table ``fs2::f0_yin`` returns
  (include/fs2hip_f0_track.h): pYIN-style candidates and a Viterbi recursion over pitch bin and voicing.
* ``fs2::dtw(x, x_lens, y, y_lens, bitmap) -> (total, K, path_i, path_j)`` — dynamic time warping under
  that cost: total f64 [B], K int32 [B], path_i / path_j int32 [B, Tx_max + Ty_max - 1] (-1 from K_b on);
  bitmap 0 / 1 / 2 = auto / LDS / global, the same bits out.
* ``fs2::path_stats(a, b, path_i, path_j, K) -> (counts, sums)`` — f64 tracks [B, T, Ch] (NaN = absent)
  read along that path: counts int64 [B, Ch, 4], sums f64 [B, Ch, 2].

Importing this module (``import fs2amd.library``, or the ``model`` drop-in package) registers the ops;
the C library itself is loaded at the first launch.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops


@torch.library.custom_op("fs2::length_regulate", mutates_args=())
def length_regulate(x: Tensor, duration: Tensor, max_len: int) -> Tuple[Tensor, Tensor]:
    out, mel_len = ops.length_regulate(x, duration, max_len if max_len > 0 else None)
    return out, mel_len


@length_regulate.register_fake
def _length_regulate_fake(x, duration, max_len):
    B, _, D = x.shape
    T = max_len if max_len > 0 else torch.library.get_ctx().new_dynamic_size()
    return x.new_empty(B, T, D), duration.new_empty(B, dtype=torch.int64)


@torch.library.custom_op("fs2::attention", mutates_args=())
def attention(qkv: Tensor, lens: Tensor, n_head: int, d_k: int, temperature: float) -> Tensor:
    return ops.attention(qkv, lens, n_head, d_k, temperature)


@attention.register_fake
def _attention_fake(qkv, lens, n_head, d_k, temperature):
    B, T, _ = qkv.shape
    return qkv.new_empty(B, T, n_head * d_k)


@torch.library.custom_op("fs2::attention_bwd", mutates_args=())
def attention_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lens: Tensor, n_head: int, d_k: int,
                  temperature: float) -> Tensor:
    return ops.attention_bwd(qkv, out, dout, lens, n_head, d_k, temperature)


@attention_bwd.register_fake
def _attention_bwd_fake(qkv, out, dout, lens, n_head, d_k, temperature):
    return qkv.new_empty(qkv.shape, dtype=torch.float32)


def _attention_setup(ctx, inputs, output):
    qkv, lens, n_head, d_k, temperature = inputs
    ctx.save_for_backward(qkv, lens, output)
    ctx.meta = (n_head, d_k, temperature)


def _attention_backward(ctx, grad):
    qkv, lens, out = ctx.saved_tensors
    dqkv = torch.ops.fs2.attention_bwd(qkv, out, grad, lens, *ctx.meta)
    return dqkv.to(qkv.dtype), None, None, None, None


torch.library.register_autograd("fs2::attention", _attention_backward, setup_context=_attention_setup)


@torch.library.custom_op("fs2::ffn", mutates_args=())
def ffn(x: Tensor, w_packed: Tensor, b1: Tensor, b2: Tensor, ln_gamma: Tensor, ln_beta: Tensor, ln_eps: float,
        lens: Optional[Tensor], ks: int, pad: int) -> Tensor:
    return ops.ffn(x, w_packed, b1, b2, ks=ks, pad=pad, ln=(ln_gamma, ln_beta, ln_eps), lens=lens)


@ffn.register_fake
def _ffn_fake(x, w_packed, b1, b2, ln_gamma, ln_beta, ln_eps, lens, ks, pad):
    return torch.empty_like(x)


@torch.library.custom_op("fs2::conv1d", mutates_args=())
def conv1d(x: Tensor, w_packed: Tensor, bias: Optional[Tensor], cin: int, ks: int, pad: int, compute: int,
           epilogue: int, out_dtype: int) -> Tensor:
    """fs2_conv1d with a plain epilogue (bias / bias + ReLU / bias + tanh / bias + leaky ReLU):
    ``nn.Conv1d`` / ``nn.Linear`` over [B, T, C] rows (the VariancePredictor / PostNet / mel_linear
    convolutions, model/modules.py:253-296, transformer/Layers.py:33-137, model/fastspeech2.py:134);
    w_packed from ops.pack_conv_weight (N = w_packed.shape[0] output channels)."""
    from . import _lib as L
    if epilogue not in (L.EPI_BIAS, L.EPI_BIAS_RELU, L.EPI_BIAS_TANH, L.EPI_BIAS_LRELU):
        raise ValueError("fs2::conv1d: plain epilogues only (residual / LayerNorm forms go through fs2amd.ops)")
    return ops.conv1d(x, w_packed, bias, cin=cin, ks=ks, pad=pad, compute=compute, epilogue=epilogue,
                      out_dtype=out_dtype)


@conv1d.register_fake
def _conv1d_fake(x, w_packed, bias, cin, ks, pad, compute, epilogue, out_dtype):
    B, T, _ = x.shape
    return x.new_empty(B, T, w_packed.shape[0], dtype=ops.torch_dtype(out_dtype))


class _StftArgs:
    """The attributes ops.mel_spectrogram reads from an STFT object, from plain op arguments."""

    def __init__(self, forward_basis, mel_basis, hop, win, max_wav_value, clip_val):
        self.forward_basis, self.mel_basis = forward_basis, mel_basis
        self.filter_length, self.hop_length, self.win_length = forward_basis.shape[-1], hop, win
        self.max_wav_value, self.clip_val = max_wav_value, clip_val


@torch.library.custom_op("fs2::mel_spectrogram", mutates_args=())
def mel_spectrogram(wav: Tensor, lens: Optional[Tensor], forward_basis: Tensor, mel_basis: Tensor, T_out: int,
                    hop: int, win: int, max_wav_value: float, clip_val: float) -> Tuple[Tensor, Tensor, Tensor]:
    if T_out < 1:
        raise ValueError("fs2::mel_spectrogram: T_out must be a positive host int")
    return ops.mel_spectrogram(wav, lens, stft=_StftArgs(forward_basis, mel_basis, hop, win, max_wav_value, clip_val),
                               T_out=T_out)


@mel_spectrogram.register_fake
def _mel_spectrogram_fake(wav, lens, forward_basis, mel_basis, T_out, hop, win, max_wav_value, clip_val):
    B = wav.shape[0]
    return (wav.new_empty(B, T_out, mel_basis.shape[0], dtype=torch.float32),
            wav.new_empty(B, T_out, dtype=torch.float32), wav.new_empty(B, dtype=torch.int64))


class _InvArgs:
    """The attributes ops.stft / ops.istft read from an STFT object, from plain op arguments."""

    def __init__(self, n_fft, hop, win, forward_basis=None, inverse_packed=None, wsum_table=None):
        self.filter_length, self.hop_length, self.win_length = n_fft, hop, win
        self.forward_basis, self.inverse_packed, self.wsum_table = forward_basis, inverse_packed, wsum_table


@torch.library.custom_op("fs2::stft", mutates_args=())
def stft(wav: Tensor, lens: Optional[Tensor], forward_basis: Tensor, T_out: int, hop: int, win: int,
         clip: bool) -> Tuple[Tensor, Tensor, Tensor]:
    if T_out < 1:
        raise ValueError("fs2::stft: T_out must be a positive host int")
    o = ops.stft(wav, lens, stft=_InvArgs(forward_basis.shape[-1], hop, win, forward_basis=forward_basis), T_out=T_out,
                 clip=clip)
    return o.spec, o.mag, o.frames


@stft.register_fake
def _stft_fake(wav, lens, forward_basis, T_out, hop, win, clip):
    B, rows = wav.shape[0], forward_basis.shape[0]
    return (wav.new_empty(B, rows, T_out, dtype=torch.float32), wav.new_empty(B, rows // 2, T_out, dtype=torch.float32),
            wav.new_empty(B, dtype=torch.int64))


@torch.library.custom_op("fs2::istft", mutates_args=())
def istft(recomb: Tensor, frames: Optional[Tensor], inverse_packed: Tensor, wsum_table: Tensor, n_out_max: int,
          hop: int, win: int) -> Tuple[Tensor, Tensor]:
    if n_out_max < 1:
        raise ValueError("fs2::istft: n_out_max must be a positive host int")
    return ops.istft(recomb, frames, stft=_InvArgs(recomb.shape[1] - 2, hop, win, inverse_packed=inverse_packed,
                                                   wsum_table=wsum_table), n_out_max=n_out_max)


@istft.register_fake
def _istft_fake(recomb, frames, inverse_packed, wsum_table, n_out_max, hop, win):
    B = recomb.shape[0]
    return recomb.new_empty(B, n_out_max, dtype=torch.float32), recomb.new_empty(B, dtype=torch.int64)


@torch.library.custom_op("fs2::pitch_targets", mutates_args=())
def pitch_targets(f0: Tensor, dur: Tensor, frames: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    o = ops.pitch_targets(f0, dur, frames)
    return o.out, o.filled, o.voiced


@pitch_targets.register_fake
def _pitch_targets_fake(f0, dur, frames):
    B, T = f0.shape
    return (f0.new_empty(B, dur.shape[1], dtype=torch.float64), f0.new_empty(B, T, dtype=torch.float64),
            f0.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("fs2::outlier_moments", mutates_args=())
def outlier_moments(values: Tensor, lens: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return tuple(ops.outlier_moments(values, lens))


@outlier_moments.register_fake
def _outlier_moments_fake(values, lens):
    B, n_max = values.shape
    return (values.new_empty(B, 2), values.new_empty(B, n_max, dtype=torch.bool),
            values.new_empty(B, dtype=torch.int64), values.new_empty(B, dtype=torch.float64),
            values.new_empty(B, dtype=torch.float64))


@torch.library.custom_op("fs2::moments_merge", mutates_args=("state",))
def moments_merge(state: Tensor, count: Tensor, mean: Tensor, m2: Tensor) -> None:
    ops.moments_merge(state, count, mean, m2)


@moments_merge.register_fake
def _moments_merge_fake(state, count, mean, m2):
    return None


@torch.library.custom_op("fs2::normalize_minmax", mutates_args=())
def normalize_minmax(values: Tensor, lens: Optional[Tensor], mean: float, std: float) -> Tuple[Tensor, Tensor]:
    return ops.normalize_minmax(values, lens, mean=mean, std=std)


@normalize_minmax.register_fake
def _normalize_minmax_fake(values, lens, mean, std):
    return values.new_empty(values.shape, dtype=torch.float64), values.new_empty(2, dtype=torch.float64)


OPS = ("length_regulate", "attention", "attention_bwd", "ffn", "conv1d", "mel_spectrogram", "stft", "istft")
# the corpus preprocessing ops (include/fs2hip_prep.h), listed on their own: OPS is the model's and the audio path's
OPS_PREP = ("pitch_targets", "outlier_moments", "moments_merge", "normalize_minmax")


@torch.library.custom_op("fs2::f0_yin", mutates_args=())
def f0_yin(wav: Tensor, lens: Optional[Tensor], sampling_rate: float, hop: int, win: int, f0_floor: float,
           f0_ceil: float, threshold: float) -> Tuple[Tensor, Tensor, Tensor]:
    return tuple(ops.f0_yin(wav, lens, sampling_rate=sampling_rate, hop_length=hop, win_length=win, f0_floor=f0_floor,
                            f0_ceil=f0_ceil, threshold=threshold, want_cmnd=True))


@f0_yin.register_fake
def _f0_yin_fake(wav, lens, sampling_rate, hop, win, f0_floor, f0_ceil, threshold):
    B, n_max = wav.shape
    F_max = n_max // hop + 1
    return (wav.new_empty(B, F_max, dtype=torch.float64), wav.new_empty(B, F_max, dtype=torch.int32),
            wav.new_empty(B, F_max, ops.f0_lags(sampling_rate, f0_floor, f0_ceil)[1] + 1, dtype=torch.float64))


# the F0 estimator (include/fs2hip_f0.h), on its own as OPS_PREP is
OPS_F0 = ("f0_yin",)


@torch.library.custom_op("fs2::f0_track", mutates_args=())
def f0_track(cmnd: Tensor, lens: Optional[Tensor], sampling_rate: float, hop: int, f0_floor: float, f0_ceil: float,
             bins_per_semitone: int, max_step: int, switch_prob: float) -> Tuple[Tensor, Tensor, Tensor]:
    return tuple(ops.f0_track(cmnd, lens, sampling_rate=sampling_rate, hop_length=hop, f0_floor=f0_floor, f0_ceil=f0_ceil,
                              bins_per_semitone=bins_per_semitone, max_step=max_step, switch_prob=switch_prob))


@f0_track.register_fake
def _f0_track_fake(cmnd, lens, sampling_rate, hop, f0_floor, f0_ceil, bins_per_semitone, max_step, switch_prob):
    B, F_max = cmnd.shape[0], cmnd.shape[1]
    return (cmnd.new_empty(B, F_max, dtype=torch.float64), cmnd.new_empty(B, F_max, dtype=torch.int32),
            cmnd.new_empty(B, dtype=torch.float64))


# the F0 tracker over that estimator's table (include/fs2hip_f0_track.h)
OPS_F0_TRACK = ("f0_track",)


@torch.library.custom_op("fs2::resample", mutates_args=())
def resample(wav: Tensor, lens: Optional[Tensor], taps: Optional[Tensor], up: int,
             down: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return tuple(ops.resample(wav, lens, up=up, down=down, taps=taps))


@resample.register_fake
def _resample_fake(wav, lens, taps, up, down):
    B, n_max = wav.shape
    M_max = (n_max * up + down - 1) // down
    return (wav.new_empty(B, M_max, dtype=torch.float64), wav.new_empty(B, M_max, dtype=torch.float32),
            wav.new_empty(B, dtype=torch.float32), wav.new_empty(B, dtype=torch.int64))


@torch.library.custom_op("fs2::peak_int16", mutates_args=())
def peak_int16(y32: Tensor, peak: Tensor, out_lens: Optional[Tensor], max_wav_value: float) -> Tensor:
    return ops.peak_int16(y32, peak, out_lens, max_wav_value=max_wav_value)


@peak_int16.register_fake
def _peak_int16_fake(y32, peak, out_lens, max_wav_value):
    return y32.new_empty(y32.shape, dtype=torch.int16)


# the resampler and the peak normalisation (include/fs2hip_resample.h), on their own as OPS_F0 is
OPS_RESAMPLE = ("resample", "peak_int16")


@torch.library.custom_op("fs2::mas", mutates_args=())
def mas(logp: Tensor, mel_lens: Optional[Tensor], text_lens: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    return tuple(ops.mas(logp, mel_lens, text_lens, want_path=True))


@mas.register_fake
def _mas_fake(logp, mel_lens, text_lens):
    B, T, Lx = logp.shape
    return (logp.new_empty(B, Lx, dtype=torch.int64), logp.new_empty(B, dtype=torch.float64),
            logp.new_empty(B, T, dtype=torch.int32))


@torch.library.custom_op("fs2::forward_sum", mutates_args=())
def forward_sum(logp: Tensor, mel_lens: Optional[Tensor], text_lens: Optional[Tensor],
                blank_logprob: float) -> Tuple[Tensor, Tensor, Tensor]:
    return tuple(ops.forward_sum(logp, mel_lens, text_lens, blank_logprob=blank_logprob))


@forward_sum.register_fake
def _forward_sum_fake(logp, mel_lens, text_lens, blank_logprob):
    B, T, Lx = logp.shape
    return (logp.new_empty((), dtype=torch.float64), logp.new_empty(B, dtype=torch.float64),
            logp.new_empty(B, T, 2 * Lx + 1, dtype=torch.float64))


@torch.library.custom_op("fs2::forward_sum_bwd", mutates_args=())
def forward_sum_bwd(logp: Tensor, mel_lens: Optional[Tensor], text_lens: Optional[Tensor], alpha: Tensor, nll: Tensor,
                    grad_out: Tensor, blank_logprob: float) -> Tensor:
    return ops.forward_sum_bwd(logp, mel_lens, text_lens, alpha, nll, grad_out, blank_logprob=blank_logprob)


@forward_sum_bwd.register_fake
def _forward_sum_bwd_fake(logp, mel_lens, text_lens, alpha, nll, grad_out, blank_logprob):
    return logp.new_empty(logp.shape)


def _forward_sum_setup(ctx, inputs, output):
    logp, mel_lens, text_lens, blank_logprob = inputs
    _, nll, alpha = output
    ctx.save_for_backward(logp, mel_lens, text_lens, alpha, nll)
    ctx.blank_logprob = blank_logprob
    ctx.set_materialize_grads(False)


def _forward_sum_backward(ctx, g_loss, g_nll, g_alpha):
    if g_loss is None:
        return None, None, None, None
    logp, mel_lens, text_lens, alpha, nll = ctx.saved_tensors
    return torch.ops.fs2.forward_sum_bwd(logp, mel_lens, text_lens, alpha, nll, g_loss, ctx.blank_logprob), None, None, None


forward_sum.register_autograd(_forward_sum_backward, setup_context=_forward_sum_setup)


# monotonic alignment search and the forward-sum loss (include/fs2hip_align.h), on their own as OPS_RESAMPLE is
OPS_ALIGN = ("mas", "forward_sum", "forward_sum_bwd")


@torch.library.custom_op("fs2::mel_cepstrum", mutates_args=())
def mel_cepstrum(mel: Tensor, lens: Optional[Tensor], basis: Tensor) -> Tensor:
    return ops.mel_cepstrum(mel, lens, basis=basis)


@mel_cepstrum.register_fake
def _mel_cepstrum_fake(mel, lens, basis):
    return mel.new_empty(mel.shape[0], mel.shape[1], basis.shape[0], dtype=torch.float64)


@torch.library.custom_op("fs2::pair_dist", mutates_args=())
def pair_dist(x: Tensor, x_lens: Optional[Tensor], y: Tensor, y_lens: Optional[Tensor]) -> Tensor:
    return ops.pair_dist(x, x_lens, y, y_lens)


@pair_dist.register_fake
def _pair_dist_fake(x, x_lens, y, y_lens):
    return x.new_empty(x.shape[0], x.shape[1], y.shape[1], dtype=torch.float64)


@torch.library.custom_op("fs2::dtw", mutates_args=())
def dtw(x: Tensor, x_lens: Optional[Tensor], y: Tensor, y_lens: Optional[Tensor],
        bitmap: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return tuple(ops.dtw(x, x_lens, y, y_lens, bitmap=("auto", "lds", "global")[bitmap]))


@dtw.register_fake
def _dtw_fake(x, x_lens, y, y_lens, bitmap):
    B, P = x.shape[0], x.shape[1] + y.shape[1] - 1
    return (x.new_empty(B, dtype=torch.float64), x.new_empty(B, dtype=torch.int32),
            x.new_empty(B, P, dtype=torch.int32), x.new_empty(B, P, dtype=torch.int32))


@torch.library.custom_op("fs2::path_stats", mutates_args=())
def path_stats(a: Tensor, b: Tensor, path_i: Tensor, path_j: Tensor, K: Tensor) -> Tuple[Tensor, Tensor]:
    return tuple(ops.path_stats(a, b, path_i, path_j, K))


@path_stats.register_fake
def _path_stats_fake(a, b, path_i, path_j, K):
    B, _, Ch = a.shape
    return a.new_empty(B, Ch, 4, dtype=torch.int64), a.new_empty(B, Ch, 2, dtype=torch.float64)


# the objective evaluation (include/fs2hip_eval.h), on its own as OPS_ALIGN is
OPS_EVAL = ("mel_cepstrum", "pair_dist", "dtw", "path_stats")
