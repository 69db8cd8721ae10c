"""Tempo and pitch perturbation of waveforms on the GPU: the rule of librosa.effects.time_stretch and
pitch_shift (an STFT, a phase vocoder, an inverse STFT, and for the pitch a polyphase resampler) in this
project's own arithmetic (include/fs2hip_pvoc.h), and ``augment_utterances``, which feeds
``build_corpus`` the copies.

* ``time_stretch`` — ops.stft -> ops.phase_vocoder -> ops.istft, cut or zero-padded to
  int(round(n / rate)) samples.
* ``pitch_shift`` — a stretch by q / p, the closest fraction p / q to 2 ** (n_steps / 12) with
  max(p, q) <= 256, then ops.resample(up=q, down=p), cut or zero-padded to the input's length.
* ``augment_utterances`` — a generator over utterance dicts: each as it is, then one copy per rate and
  per step.

The STFT is the model's (1024 / 256): other geometries are refused by the kernels. It is librosa's
rule, not librosa's bits. The running phase starts from the first frame, which the STFT fills by
reflect padding; at rates below 1 that frame's phases stay in the output and can lower its level
(DESIGN 9.9 has figures): it is an augmentation, not a transparent time-scale modification.
"""
import math

import numpy as np
import torch

PITCH_FRACTION_LIMIT = 256  # max(p, q): 20 * max(p, q) + 1 float64 taps stay inside the resampler's LDS staging


def rescale_durations(durations, rate, n_new, hop_length):
    """Durations (frames per phoneme) of an utterance stretched by ``rate`` to n_new samples: over the
    cumulative boundaries c_k, c'_k = min(T', floor(c_k / rate + 0.5)) with T' = 1 + n_new // hop_length,
    the frames of the new mel; the new durations are the differences (int64, never negative)."""
    c = np.cumsum(np.asarray(durations, dtype=np.int64))
    T_new = 1 + int(n_new) // int(hop_length)
    cn = np.minimum(T_new, np.floor(c / float(rate) + 0.5).astype(np.int64))
    return np.diff(np.concatenate([np.zeros(1, dtype=np.int64), cn])).astype(np.int64)


def pitch_fraction(n_steps, limit=PITCH_FRACTION_LIMIT):
    """(p, q) in lowest terms, max(p, q) <= limit, with p / q closest to 2 ** (n_steps / 12) (the smallest
    q on a tie)."""
    f = 2.0 ** (float(n_steps) / 12.0)
    best = None
    for q in range(1, limit + 1):
        lo = int(math.floor(f * q))
        for p in (lo, lo + 1):
            p = min(max(p, 1), limit)
            err = abs(p / q - f)
            if best is None or err < best[0]:
                best = (err, p, q)
    g = math.gcd(best[1], best[2])
    return best[1] // g, best[2] // g


def _float_wavs(wavs):
    wavs = [np.asarray(w) for w in wavs]
    if any(w.ndim != 1 or w.dtype not in (np.int16, np.float32) for w in wavs):
        raise ValueError("fs2amd: waveforms are 1-D int16 or float32 arrays")
    return [w.astype(np.float32) / np.float32(32768.0) if w.dtype == np.int16 else w for w in wavs]


def _per_wav(values, n, name):
    values = [values] * n if np.ndim(values) == 0 else list(values)
    if len(values) != n:
        raise ValueError(f"fs2amd: one {name} per waveform, or one number for all")
    return [float(v) for v in values]


def _stretch(wavs, rates, stft, dev):
    """The stretch of a packed batch on the device: (rows f32 [B, W], zero past every row's own output,
    the target lengths int(round(n / rate))). One launch each of stft, phase_vocoder, istft."""
    from . import ops
    from .preprocess import _pack

    stft = getattr(stft, "stft_fn", stft)
    hop, n_fft = int(stft.hop_length), int(stft.filter_length)
    for r in rates:
        if not (r > 0.0 and math.isfinite(r)):
            raise ValueError(f"fs2amd: a stretch rate is a positive finite number, got {r!r}")
    wav, lens = _pack(wavs, np.float32)
    targets = [int(round(int(n) / r)) for n, r in zip(lens, rates)]
    T = [int(ops.mel_frames(int(n), hop, n_fft)) for n in lens]
    J = [ops.pvoc_frames(t, r) for t, r in zip(T, rates)]
    J_max = max(J + [1])
    spec = ops.stft(torch.from_numpy(wav).to(dev), torch.from_numpy(lens), stft=stft, T_out=max(T + [1]),
                    want=("spec",)).spec
    recomb, _ = ops.phase_vocoder(spec, torch.tensor(T, dtype=torch.int64), torch.tensor(rates, dtype=torch.float64),
                                  J_max=J_max)
    width = max(targets + [hop * (J_max - 1), 1])
    rows, _ = ops.istft(recomb, torch.tensor(J, dtype=torch.int64), stft=stft, n_out_max=width)
    return rows, targets


def time_stretch(wavs, rates, *, stft, device=None):
    """A list of 1-D int16 / float32 waveforms, each played ``rate`` times as fast at the same pitch
    (rate < 1: slower and longer): float32 arrays of int(round(len / rate)) samples. rates: one number,
    or one per waveform. int16 input is widened by / 32768 first. stft: a fs2amd.audio.STFT or
    TacotronSTFT on the GPU (1024 / 256). The whole list is one batch: one STFT, one phase vocoder
    (include/fs2hip_pvoc.h), one inverse STFT; the inverse gives 256 * (frames - 1) samples, which are
    cut or zero-padded to the length. A waveform of at most 512 samples has no frames and comes back as
    zeros. The result of a waveform does not depend on the others in the list."""
    from .preprocess import _device

    dev = _device(device)
    wavs = _float_wavs(wavs)
    rates = _per_wav(rates, len(wavs), "rate")
    if not wavs:
        return []
    rows, targets = _stretch(wavs, rates, stft, dev)
    rows = rows.cpu().numpy()
    return [rows[b, :n].copy() for b, n in enumerate(targets)]


def pitch_shift(wavs, n_steps, *, stft, device=None):
    """A list of 1-D int16 / float32 waveforms, each shifted by ``n_steps`` semitones (one number, or one
    per waveform; fractions allowed) at the same length: float32 arrays. With p / q = ``pitch_fraction``
    (n_steps), the waveform is stretched by the rate q / p (as ``time_stretch``, all of the list in one
    batch) and resampled by ops.resample(up=q, down=p) (one launch per distinct fraction), then cut or
    zero-padded to its own length. The shift is therefore by p / q exactly, within 0.2 % of the
    semitone ratio."""
    from . import ops
    from .audio import resample_taps
    from .preprocess import _device

    dev = _device(device)
    wavs = _float_wavs(wavs)
    steps = _per_wav(n_steps, len(wavs), "n_steps")
    if not wavs:
        return []
    fracs = [pitch_fraction(s) for s in steps]
    rows, targets = _stretch(wavs, [q / p for p, q in fracs], stft, dev)
    groups = {}
    for b, pq in enumerate(fracs):
        groups.setdefault(pq, []).append(b)
    res = [None] * len(wavs)
    for (p, q), idx in groups.items():
        sel = rows if len(idx) == len(wavs) else rows[torch.tensor(idx, device=dev)]
        lens = torch.tensor([targets[b] for b in idx], dtype=torch.int64)
        if p == q:
            y = sel.cpu().numpy()
        else:
            taps = torch.from_numpy(resample_taps(q, p) * q).to(dev)
            y = ops.resample(sel, lens, up=q, down=p, taps=taps, want_y=False).y32.cpu().numpy()
        for j, b in enumerate(idx):
            n = len(wavs[b])
            out = np.zeros(n, dtype=np.float32)
            m = min(n, y.shape[1])
            out[:m] = y[j, :m]
            res[b] = out
    return res


def _suffix_rate(rate):
    return f"_ts{rate:.2f}"


def _suffix_steps(steps):
    return f"_ps{steps:+g}"


def augment_utterances(utterances, *, rates=(), n_steps=(), stft, batch_size=16):
    """A generator for ``build_corpus``: every utterance dict as it is, then one copy per rate of
    ``rates`` (``time_stretch``) and per step of ``n_steps`` (``pitch_shift``), in that order. A copy has
    its ``basename`` suffixed ("_ts0.90", "_ps+2"), its ``wav`` replaced, ``f0`` set to None (so that it
    is estimated from the new audio) and everything else kept, but for the ``durations`` of a stretch:
    those follow ``rescale_durations`` with the STFT's hop, so that they fit the new mel; None stays
    None (the aligner supplies them). The copy of an int16 waveform is int16 again (rounded, saturated),
    so that a batch of ``build_corpus`` stays of one dtype. Utterances are stretched batch_size at a
    time, one launch sequence per rate and step. ``start`` / ``end`` refer to the waveform's own time
    axis, which a stretch changes: such an utterance is refused when rates are given."""
    from .preprocess import _device

    rates, n_steps = [float(r) for r in rates], [float(s) for s in n_steps]
    names = [_suffix_rate(r) for r in rates] + [_suffix_steps(s) for s in n_steps]
    if len(set(names)) != len(names):
        raise ValueError(f"fs2amd: two copies would share a name: {names}")
    hop = int(getattr(stft, "stft_fn", stft).hop_length)
    dev = _device(stft.mel_basis.device if hasattr(stft, "mel_basis") else stft.forward_basis.device)

    def like(u, w):
        if np.asarray(u["wav"]).dtype != np.int16:
            return w
        return np.clip(np.rint(w.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)

    def flush(batch):
        wavs = [np.asarray(u["wav"]) for u in batch]
        copies = [[] for _ in batch]
        for u in batch:
            if rates and (u.get("start") is not None or u.get("end") is not None):
                raise ValueError(f"fs2amd: {u['basename']} brings start / end; cut it before it is stretched")
        for r in rates:
            for b, w in enumerate(time_stretch(wavs, r, stft=stft, device=dev)):
                u = batch[b]
                d = u.get("durations")
                copies[b].append(dict(u, basename=u["basename"] + _suffix_rate(r), wav=like(u, w), f0=None,
                                      durations=None if d is None else rescale_durations(d, r, len(w), hop)))
        for s in n_steps:
            for b, w in enumerate(pitch_shift(wavs, s, stft=stft, device=dev)):
                u = batch[b]
                copies[b].append(dict(u, basename=u["basename"] + _suffix_steps(s), wav=like(u, w), f0=None))
        for u, cs in zip(batch, copies):
            yield u
            yield from cs

    batch = []
    for u in utterances:
        batch.append(u)
        if len(batch) == batch_size:
            yield from flush(batch)
            batch = []
    if batch:
        yield from flush(batch)
