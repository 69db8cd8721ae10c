"""From waveforms, F0 contours and phone alignments to a trainable corpus directory: what the
reference's preprocessor/preprocessor.py does between feature extraction and ``stats.json``.

* ``get_alignment`` — :327-365 over ``(start, end, label)`` intervals (host code).
* ``prepare_wavs`` — the prepare_align step before it (preprocessor/esd_chinese.py:145-147): raw audio
  at any rate to peak-normalised int16 at the configuration's (include/fs2hip_resample.h).
* ``trim_silence`` / ``split_silence`` — the rule of librosa.effects.trim / split in this project's own
  float64 arithmetic (include/fs2hip_vad.h): what stands in for the TextGrid's first and last phone
  (:245-249) where there is no TextGrid.
* ``f0_contour`` — the contour the reference takes from pyworld (:255-261), here from YIN on the GPU.
* ``pitch_targets`` — :263-291: crop, interpolate over unvoiced frames, phoneme mean.
* ``remove_outlier`` / ``CorpusStats`` — :367-375 and the ``StandardScaler.partial_fit`` calls of
  :152-155: the IQR fence per utterance and a running mean / variance kept on the device.
* ``normalize`` — :377-388 with the switches of :161-173.
* ``build_corpus`` — the directory layout of :183-222 and :304-325.

The arithmetic runs in the kernels of include/fs2hip_prep.h (float64, uncontracted; see the header
for what is exact). The F0 contour per utterance, float64 and 0 where unvoiced, is either an input
(as ``pyworld.stonemask`` returns it) or estimated from the waveform by the kernel of
include/fs2hip_f0.h. That estimator is YIN, not WORLD's DIO + StoneMask: same time grid, length
and range, other values, so ``stats.json`` built from it differs from a WORLD-built corpus's and a
checkpoint should be used with targets from the estimator it was trained on. TextGrid files are
not read.
"""
import json
import os
import random

import numpy as np
import torch

SIL_PHONES = ("sil", "sp", "spn")


def get_alignment(intervals, sampling_rate, hop_length):
    """preprocessor.py:327-365. intervals: (start_time, end_time, label) in tier order. Returns
    (phones, durations, start_time, end_time): leading silences dropped, trailing ones cut off,
    inner ones kept; durations in frames. An all-silence tier gives ([], [], 0, 0): the caller drops
    an utterance with start >= end."""
    phones, durations = [], []
    start_time, end_time, end_idx = 0, 0, 0
    for s, e, p in intervals:
        if not phones:
            if p in SIL_PHONES:
                continue
            start_time = s
        phones.append(p)
        if p not in SIL_PHONES:
            end_time = e
            end_idx = len(phones)
        durations.append(int(np.round(e * sampling_rate / hop_length) - np.round(s * sampling_rate / hop_length)))
    return phones[:end_idx], durations[:end_idx], start_time, end_time


def _device(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("fs2amd: preprocessing runs on the HIP kernels only (no CPU fallback)")
    return dev


def _pack(arrays, dtype):
    """A list of 1-D arrays -> (host [B, n_max >= 1] zero-padded, int64 lens [B])."""
    lens = np.array([len(a) for a in arrays], dtype=np.int64)
    out = np.zeros((len(arrays), max(int(lens.max(initial=0)), 1)), dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out, lens


def _common_dtype(arrays):
    """float32 when every array is float32, else float64 (what numpy would promote to)."""
    arrays = [np.asarray(a) for a in arrays]
    if any(a.ndim != 1 for a in arrays):
        raise ValueError("fs2amd: value tracks are 1-D arrays")
    return arrays, (np.float32 if arrays and all(a.dtype == np.float32 for a in arrays) else np.float64)


def pitch_targets(f0_list, durations, *, device=None, return_filled=False):
    """Phoneme-level pitch targets of a batch: f0_list float64 contours (0 = unvoiced), durations
    integer arrays (frames per phoneme). Returns a list with a float64 [L_b] array per utterance, or
    None where the reference drops it (at most one voiced frame within sum(duration)).
    return_filled: also the interpolated frame-level contours [min(len(f0), sum(d))] (None likewise)."""
    from . import ops

    dev = _device(device)
    if len(f0_list) != len(durations):
        raise ValueError("fs2amd: one duration array per contour")
    f0, frames = _pack([np.asarray(f, dtype=np.float64) for f in f0_list], np.float64)
    dur, n_ph = _pack([np.asarray(d, dtype=np.int64) for d in durations], np.int64)
    o = ops.pitch_targets(torch.from_numpy(f0).to(dev), torch.from_numpy(dur).to(dev), torch.from_numpy(frames))
    out, filled, voiced = o.out.cpu().numpy(), o.filled.cpu().numpy(), o.voiced.cpu().numpy()
    res, fil = [], []
    for b in range(len(f0_list)):
        keep = voiced[b] > 1
        n = min(int(frames[b]), int(np.maximum(dur[b], 0).sum()))
        res.append(out[b, :n_ph[b]].copy() if keep else None)
        fil.append(filled[b, :n].copy() if keep else None)
    return (res, fil) if return_filled else res


F0_DEFAULTS = {"f0_floor": 71.0, "f0_ceil": 800.0, "threshold": 0.1, "win_length": 1024}


F0_METHODS = ("yin", "track")


def _f0_rows(wav_dev, lens, method="yin", **kw):
    """ops.f0_yin over an uploaded batch -> the float64 contours [lens[b] // hop + 1] on the host.
    method "track": the same launch with its cmnd table kept on the device, then ops.f0_track over it."""
    from . import ops

    if method not in F0_METHODS:
        raise ValueError(f"fs2amd: the F0 method is one of {F0_METHODS}, got {method!r}")
    lens_t = torch.from_numpy(np.asarray(lens, dtype=np.int64))
    if method == "yin":
        f0 = ops.f0_yin(wav_dev, lens_t, want_tau=False, **kw).f0
    else:
        lens_dev = lens_t.to(wav_dev.device)
        cmnd = ops.f0_yin(wav_dev, lens_dev, want_tau=False, want_cmnd=True, **kw).cmnd
        f0 = ops.f0_track(cmnd, lens_dev, sampling_rate=kw["sampling_rate"], hop_length=kw["hop_length"],
                          f0_floor=kw["f0_floor"], f0_ceil=kw["f0_ceil"], want_score=False).f0
    f0 = f0.cpu().numpy()
    return [f0[b, :int(n) // int(kw["hop_length"]) + 1].copy() for b, n in enumerate(lens)]


def f0_contour(wavs, *, sampling_rate, hop_length, win_length=1024, f0_floor=71.0, f0_ceil=800.0, threshold=0.1,
               method="yin", device=None):
    """F0 contours of a list of 1-D int16 / float32 waveforms: a list of float64 arrays of length
    len(w) // hop_length + 1, one value per hop at sample k * hop_length, 0 where unvoiced: the
    grid, length and range (71-800 Hz) of the reference's pyworld call, but YIN (include/fs2hip_f0.h),
    so the values are not WORLD's. A batch with any float32 waveform is processed as float32.
    method "yin": every frame decided on its own against ``threshold``. method "track": one path
    through the utterance over the same table (include/fs2hip_f0_track.h, pYIN-style; ``threshold``
    plays no part): fewer octave errors and dropped frames, other values again."""
    dev = _device(device)
    wavs = [np.asarray(w) for w in wavs]
    if any(w.ndim != 1 or w.dtype not in (np.int16, np.float32) for w in wavs):
        raise ValueError("fs2amd: waveforms are 1-D int16 or float32 arrays")
    if not wavs:
        return []
    wav, lens = _pack(wavs, np.int16 if all(w.dtype == np.int16 for w in wavs) else np.float32)
    return _f0_rows(torch.from_numpy(wav).to(dev), lens, sampling_rate=sampling_rate, hop_length=hop_length,
                    win_length=win_length, f0_floor=f0_floor, f0_ceil=f0_ceil, threshold=threshold, method=method)


def _vad_params(top_db, dtype):
    """(threshold, floor) of include/fs2hip_vad.h for top_db and a waveform dtype: 10 ** (-top_db / 10)
    and librosa's amin on amplitude, (1e-5 * full_scale) ** 2 with full_scale 32768 for int16, 1 for float32."""
    return 10 ** (-float(top_db) / 10), (1e-5 * (32768.0 if dtype == np.int16 else 1.0)) ** 2


def _vad_batch(wav_dev, lens, dtype, *, top_db, frame_length, hop_length, min_silence, margin):
    """ops.frame_power + ops.activity_intervals over an uploaded batch: (count, intervals, trim) on the device."""
    from . import ops

    lens_dev = torch.from_numpy(np.asarray(lens, dtype=np.int64)).to(wav_dev.device)
    P, Pmax, _ = ops.frame_power(wav_dev, lens_dev, frame_length=frame_length, hop_length=hop_length)
    threshold, floor = _vad_params(top_db, dtype)
    _, count, intervals, trim = ops.activity_intervals(P, Pmax, lens_dev, threshold=threshold, floor=floor,
                                                       hop_length=hop_length, min_silence=min_silence, margin=margin,
                                                       n_max=wav_dev.shape[1])
    return count, intervals, trim


def _wav_list(wavs):
    wavs = [np.asarray(w) for w in wavs]
    if any(w.ndim != 1 or w.dtype not in (np.int16, np.float32) for w in wavs):
        raise ValueError("fs2amd: waveforms are 1-D int16 or float32 arrays")
    return wavs


def trim_silence(wavs, *, top_db=60.0, frame_length=2048, hop_length=512, min_silence=1, margin=0, device=None):
    """Leading and trailing silence cut from a list of 1-D int16 / float32 waveforms by the rule of
    librosa.effects.trim (the defaults are librosa's): a centred, zero-padded frame is active where its
    power exceeds the utterance's largest frame power less top_db decibels; the waveform is cut to
    [first active frame * hop_length - margin, (last active frame + 1) * hop_length + margin), clamped.
    Returns (the trimmed arrays, int64 [B, 2] of (start, end)). It is librosa's rule in this project's
    float64 arithmetic (include/fs2hip_vad.h), not librosa's bits. Every waveform is judged in its own
    dtype: int16 against full scale 32768, float32 against 1.0; each dtype is one batch on the device.
    min_silence > 1 also counts inner pauses shorter than that many frames as speech (which moves
    nothing here; see ``split_silence``). A waveform without an active frame comes back empty."""
    from . import ops

    dev = _device(device)
    wavs = _wav_list(wavs)
    res, se = [None] * len(wavs), np.zeros((len(wavs), 2), dtype=np.int64)
    for dtype in (np.int16, np.float32):
        idx = [b for b, w in enumerate(wavs) if w.dtype == dtype]
        if not idx:
            continue
        wav, lens = _pack([wavs[b] for b in idx], dtype)
        wav_dev = torch.from_numpy(wav).to(dev)
        _, _, trim = _vad_batch(wav_dev, lens, dtype, top_db=top_db, frame_length=frame_length, hop_length=hop_length,
                                min_silence=min_silence, margin=margin)
        rows, out_lens = ops.cut_rows(wav_dev, trim[:, 0].contiguous(), trim[:, 1].contiguous())
        rows, out_lens, trim = rows.cpu().numpy(), out_lens.cpu().numpy(), trim.cpu().numpy()
        for j, b in enumerate(idx):
            res[b] = rows[j, :int(out_lens[j])].copy()
            se[b] = trim[j]
    return res, se


def split_silence(wavs, *, top_db=60.0, frame_length=2048, hop_length=512, min_silence=1, device=None):
    """The non-silent intervals of a list of 1-D int16 / float32 waveforms by the rule of
    librosa.effects.split: a list of int64 [k_b, 2] arrays of [start, end) in samples, one row per maximal
    run of active frames, [first frame * hop_length, min(len, (last frame + 1) * hop_length)).
    min_silence: inner pauses shorter than that many frames do not split (1: librosa's behaviour).
    Arithmetic and dtypes as ``trim_silence``."""
    dev = _device(device)
    wavs = _wav_list(wavs)
    res = [None] * len(wavs)
    for dtype in (np.int16, np.float32):
        idx = [b for b, w in enumerate(wavs) if w.dtype == dtype]
        if not idx:
            continue
        wav, lens = _pack([wavs[b] for b in idx], dtype)
        count, intervals, _ = _vad_batch(torch.from_numpy(wav).to(dev), lens, dtype, top_db=top_db,
                                         frame_length=frame_length, hop_length=hop_length, min_silence=min_silence,
                                         margin=0)
        count, intervals = count.cpu().numpy(), intervals.cpu().numpy()
        for j, b in enumerate(idx):
            res[b] = intervals[j, :int(count[j])].copy()
    return res


def prepare_wavs(wavs, rates, *, sampling_rate, max_wav_value=32768.0, device=None, trim_db=None,
                 trim_frame_length=2048, trim_hop_length=512, trim_margin=0, lufs=None, lufs_peak_ceiling=None):
    """The reference's prepare_align arithmetic (preprocessor/esd_chinese.py:145-147) for a list of
    1-D int16 / float32 waveforms at the source rates ``rates`` (one per waveform, or one number for
    all): resampled to ``sampling_rate``, divided by the peak, scaled by max_wav_value and cut to
    int16. Returns a list of int16 arrays of ceil(len * up / down) samples, in input order. One
    ops.resample + ops.peak_int16 pair per distinct source rate; a waveform already at
    ``sampling_rate`` is only peak-normalised, as the reference does to every file. The resampler is
    scipy.signal.resample_poly's (include/fs2hip_resample.h), not librosa's soxr_hq; a positive peak
    comes out as 32767 where the reference's cast wraps. An all-zero waveform stays zero.
    trim_db: None, or the top_db of ``trim_silence``: every group is then trimmed on the device after
    the int16 pass and before the copy back (frames of trim_frame_length every trim_hop_length,
    trim_margin samples kept on either side); on int16 rows every sum of the frame power is exact.
    lufs: None, or a target in LUFS: every group is then brought to that integrated loudness on the
    device (``fs2amd.loudness``: BS.1770 K-weighting and gating at ``sampling_rate``, one gain per
    waveform, int16 rounded to nearest and saturated) after the int16 pass and after the trim, before
    the copy back. lufs_peak_ceiling: None, or the largest |sample| allowed as a fraction of full
    scale; the gain is lowered where it would exceed that. A waveform with no block above the gates
    (shorter than 400 ms, or silent) keeps its peak-normalised samples. None runs nothing more."""
    from . import ops
    from .audio import resample_ratio, resample_taps

    dev = _device(device)
    kw = None
    if lufs is not None:
        from . import loudness

        kw = loudness.KWeighting(sampling_rate, dev)
    wavs = [np.asarray(w) for w in wavs]
    if any(w.ndim != 1 or w.dtype not in (np.int16, np.float32) for w in wavs):
        raise ValueError("fs2amd: waveforms are 1-D int16 or float32 arrays")
    rates = [rates] * len(wavs) if np.ndim(rates) == 0 else list(rates)
    if len(rates) != len(wavs):
        raise ValueError("fs2amd: one source rate per waveform")
    groups = {}  # source rate -> indices, in order of first appearance
    for b, r in enumerate(rates):
        if int(r) != r:
            raise ValueError(f"fs2amd: sampling rates must be integers, got {r!r}")
        groups.setdefault(int(r), []).append(b)
    res = [None] * len(wavs)
    for rate, idx in groups.items():
        up, down = resample_ratio(sampling_rate, rate)
        group = [wavs[b] for b in idx]
        wav, lens = _pack(group, np.int16 if all(w.dtype == np.int16 for w in group) else np.float32)
        taps = None if up == down == 1 else torch.from_numpy(resample_taps(up, down) * up).to(dev)
        o = ops.resample(torch.from_numpy(wav).to(dev), torch.from_numpy(lens), up=up, down=down, taps=taps, want_y=False)
        q = ops.peak_int16(o.y32, o.peak, o.out_lens, max_wav_value=max_wav_value)
        out_lens = [ops.resample_out_len(int(n), up, down) for n in lens]
        if trim_db is not None:
            _, _, trim = _vad_batch(q, out_lens, np.int16, top_db=trim_db, frame_length=trim_frame_length,
                                    hop_length=trim_hop_length, min_silence=1, margin=trim_margin)
            q, cut_lens = ops.cut_rows(q, trim[:, 0].contiguous(), trim[:, 1].contiguous())
            out_lens = cut_lens.cpu().tolist()
        if kw is not None:
            ceiling = None if lufs_peak_ceiling is None else float(lufs_peak_ceiling) * 32768.0
            _, r = loudness.normalize_batch(q, torch.as_tensor(out_lens, dtype=torch.int64).to(dev), kw,
                                            target_lufs=lufs, peak_ceiling=ceiling)
            q = r.q
        q = q.cpu().numpy()
        for j, b in enumerate(idx):
            res[b] = q[j, :out_lens[j]].copy()
    return res


def _fence(arrays, dev):
    """ops.outlier_moments over a list of tracks: (OutlierOut, host lens, packed device values)."""
    from . import ops

    arrays, dtype = _common_dtype(arrays)
    vals, lens = _pack(arrays, dtype)
    v = torch.from_numpy(vals).to(dev)
    return ops.outlier_moments(v, torch.from_numpy(lens)), lens, arrays


def remove_outlier(values, *, device=None):
    """preprocessor.py:367-375: the values strictly inside [p25 - 1.5 iqr, p75 + 1.5 iqr], in order,
    in the input's dtype (float32 stays float32; anything else is taken as float64)."""
    o, lens, arrays = _fence([values], _device(device))
    return arrays[0][o.inlier[0, :lens[0]].cpu().numpy()]


class CorpusStats:
    """The running mean and variance of the reference's StandardScaler over outlier-free values
    (preprocessor.py:125-126, :152-155), kept on the device: ``partial_fit`` makes no device-to-host
    copy; the attributes read the three-number state when asked."""

    def __init__(self, device=None):
        self.device = _device(device)
        self.state = torch.zeros(3, dtype=torch.float64, device=self.device)

    def partial_fit(self, arrays):
        """The IQR fence of every array, the moments of its inliers, and their merge into the state,
        in list order; an array without inliers (or an empty list) leaves the state as it is."""
        from . import ops

        if len(arrays) == 0:
            return self
        o, _, _ = _fence(arrays, self.device)
        ops.moments_merge(self.state, o.count, o.mean, o.m2)
        return self

    def _host(self):
        n, mean, m2 = self.state.cpu().tolist()
        return n, mean, m2

    @property
    def n_samples_seen_(self):
        return int(self._host()[0])

    @property
    def mean_(self):
        return self._host()[1]

    @property
    def var_(self):
        n, _, m2 = self._host()
        return m2 / n if n > 0 else 0.0

    @property
    def scale_(self):
        """sqrt(var_), and 1.0 where the variance is 0, as sklearn's _handle_zeros_in_scale."""
        var = self.var_
        return float(np.sqrt(var)) if var > 0.0 else 1.0


def normalize(arrays, mean, std, *, device=None):
    """preprocessor.py:377-388 over a list of tracks: ((v - mean) / std per track as float64, min,
    max) with min / max over every value, outliers included. With mean = 0 and std = 1 (the
    reference's way of switching normalisation off) the arrays come back as they are, in their own
    dtype, as ``(values - 0) / 1`` leaves them."""
    from . import ops

    arrays, dtype = _common_dtype(arrays)
    if not arrays:
        return [], float(np.finfo(np.float64).max), float(np.finfo(np.float64).min)
    vals, lens = _pack(arrays, dtype)
    out, mm = ops.normalize_minmax(torch.from_numpy(vals).to(_device(device)), torch.from_numpy(lens), mean=mean, std=std)
    vmin, vmax = mm.cpu().tolist()
    if mean == 0 and std == 1:
        return [a.copy() for a in arrays], vmin, vmax
    out = out.cpu().numpy()
    return [out[b, :lens[b]].copy() for b in range(len(arrays))], vmin, vmax


def _aligned_durations(batch, wav_dev, lens, stft, aligner):
    """The batch's durations: an utterance's own where it brings them, the aligner's over the mel of
    the uploaded waveform where it does not."""
    from . import ops

    durs = [u.get("durations") for u in batch]
    need = [b for b, d in enumerate(durs) if d is None]
    if need:
        mel, _, frames = ops.mel_spectrogram(wav_dev, torch.from_numpy(np.asarray(lens, dtype=np.int64)), stft=stft)
        mel, frames = mel.cpu().numpy(), frames.cpu().numpy()
        ids = [np.array([aligner.symbols[p] for p in batch[b]["phones"]], dtype=np.int64) for b in need]
        got = aligner.durations(ids, [mel[b, :int(frames[b])] for b in need])
        for b, d in zip(need, got):
            durs[b] = d
    return [np.asarray(d, dtype=np.int64) for d in durs]


def build_corpus(out_dir, utterances, preprocess_config, *, stft, val_size=None, seed=1234, batch_size=16,
                 emotions=None, aligner=None, f0_method="yin", trim_db=None, trim_margin=0, lufs=None):
    """Write a preprocessed corpus directory (preprocessor.py:116-224, :304-325) from utterances, an
    iterable of dicts with ``basename``, ``speaker``, ``phones`` (list of labels), ``raw_text``,
    ``aux`` (the metadata tail, e.g. "emotion|arousal|valence"), ``wav`` (1-D float32 in [-1, 1] or
    int16), ``f0`` (float64 contour at the STFT's hop, 0 = unvoiced) and ``durations`` (frames per
    phoneme). stft: a fs2amd.audio.TacotronSTFT on the GPU. val_size: None = the configuration's.
    An utterance without ``f0`` (or with None) gets its contour from ``ops.f0_yin`` over the batch
    already uploaded for the features, at the configuration's sampling rate and hop, with the
    defaults of ``f0_contour`` unless preprocess_config["preprocessing"]["pitch_extraction"] sets
    ``f0_floor`` / ``f0_ceil`` / ``threshold`` / ``win_length``. f0_method: "yin" or "track", as
    ``f0_contour``'s method; a ``stats.json`` built with one goes with checkpoints trained on its targets.
    Three more optional keys: ``sampling_rate``, the rate of ``wav`` when it is raw audio: such an
    utterance goes through ``prepare_wavs`` first (resampled to the configuration's rate and
    peak-normalised to int16); ``start`` / ``end`` in seconds: the waveform (prepared or not) is cut
    to ``[int(sr * start):int(sr * end)]`` as preprocessor.py:247-249 does, and ``durations`` and
    ``f0`` refer to the cut waveform. An utterance with none of them is processed as it is.
    aligner: None, or an object with ``symbols`` (phoneme label -> id) and ``durations(phone_ids_list,
    mels_list)`` such as ``fs2amd.align.Aligner``: an utterance without ``durations`` (or with None)
    then gets them from it. The mel of the prepared, cut waveform is computed first, over the batch
    already uploaded; the aligner's durations sum to its frame count. Utterances that bring
    ``durations`` go exactly as without an aligner, and a batch may mix both.
    trim_db: None, or the top_db of ``trim_silence``: an utterance that brings neither ``start`` nor
    ``end`` then has its leading and trailing silence cut (after ``prepare_wavs``, before anything else;
    trim_margin samples kept on either side) with frames of the configuration's win_length every
    hop_length, so that the cut lies on the mel grid. Its ``durations`` and ``f0``, if it brings any,
    refer to the trimmed waveform: durations that sum to more frames than its mel has raise a ValueError
    (everywhere else durations are expected to fit, as ``extract_features`` says). An utterance that
    trims to nothing is dropped, as an all-silence TextGrid is.
    lufs: None, or a target in LUFS handed to ``prepare_wavs`` for the utterances that go through it
    (the ones that name their ``sampling_rate``): they are loudness-normalised after the peak
    normalisation, before the ``start`` / ``end`` cut and the trim; the gating makes the measurement
    indifferent to the silence those remove. None changes nothing.

    Utterances go through extract_features, pitch_targets and two CorpusStats in batches of
    batch_size; the ones the reference drops (at most one voiced frame) are left out. Pitch and
    energy are phoneme-level or frame-level and normalised or not as
    preprocess_config["preprocessing"] says. Written: duration/ (int64), pitch/ (float64), energy/
    (float64 when normalised, else float32), mel/ ([T, n_mel] float32) as <speaker>-<kind>-<basename>.npy,
    stats.json ([min, max, mean, std] for pitch and energy), speakers.json (speaker -> index in
    order of first appearance), emotions.json when ``emotions`` is given, and train.txt / val.txt:
    the lines shuffled by random.Random(seed), the first val_size to val.txt. Returns the lines."""
    from .audio import extract_features

    pp = preprocess_config["preprocessing"]
    dev = stft.mel_basis.device
    if val_size is None:
        val_size = pp["val_size"]
    ph_pitch, ph_energy = pp["pitch"]["feature"] == "phoneme_level", pp["energy"]["feature"] == "phoneme_level"
    for feat in (pp["pitch"]["feature"], pp["energy"]["feature"]):
        if feat not in ("phoneme_level", "frame_level"):
            raise ValueError(f"fs2amd: unknown feature level {feat!r}")
    for kind in ("mel", "pitch", "energy", "duration"):
        os.makedirs(os.path.join(out_dir, kind), exist_ok=True)
    f0_kw = dict(F0_DEFAULTS, **pp.get("pitch_extraction", {}))
    if f0_method not in F0_METHODS:
        raise ValueError(f"fs2amd: f0_method is one of {F0_METHODS}, got {f0_method!r}")
    sr = pp["audio"]["sampling_rate"]
    pitch_stats, energy_stats = CorpusStats(dev), CorpusStats(dev)
    speakers, lines, kept = {}, [], []  # kept: (speaker, basename, pitch, energy)

    def raw_wavs(batch):
        """The batch's waveforms at the configuration's rate: prepare_wavs for the utterances that
        name their own rate, then the alignment's cut (preprocessor.py:247-249)."""
        wavs = [np.asarray(u["wav"]) for u in batch]
        own = [b for b, u in enumerate(batch) if u.get("sampling_rate") is not None]
        if own:
            ready = prepare_wavs([wavs[b] for b in own], [batch[b]["sampling_rate"] for b in own], sampling_rate=sr,
                                 max_wav_value=pp["audio"].get("max_wav_value", 32768.0), device=dev,
                                 **({} if lufs is None else {"lufs": lufs}))
            for b, w in zip(own, ready):
                wavs[b] = w
        for b, u in enumerate(batch):
            start, end = u.get("start"), u.get("end")
            if start is not None or end is not None:
                wavs[b] = wavs[b][None if start is None else int(sr * start):None if end is None else int(sr * end)]
        if trim_db is not None:
            free = [b for b, u in enumerate(batch) if u.get("start") is None and u.get("end") is None]
            if free:
                cut, _ = trim_silence([wavs[b] for b in free], top_db=trim_db, frame_length=pp["stft"]["win_length"],
                                      hop_length=pp["stft"]["hop_length"], margin=trim_margin, device=dev)
                for b, w in zip(free, cut):
                    wavs[b] = w
                    d = batch[b].get("durations")
                    frames = 1 + len(w) // pp["stft"]["hop_length"]
                    if d is not None and len(w) > 0 and int(np.sum(d)) > frames:
                        raise ValueError(f"fs2amd: the durations of {batch[b]['basename']} sum to {int(np.sum(d))} frames; "
                                         f"its trimmed waveform has {frames}")
        return wavs

    def flush(batch):
        wavs = raw_wavs(batch)
        if trim_db is not None:  # trimmed to nothing: dropped, as preprocessor.py:245-246 drops start >= end
            keep = [b for b, w in enumerate(wavs) if len(w) > 0]
            batch, wavs = [batch[b] for b in keep], [wavs[b] for b in keep]
            if not batch:
                return
        wdtype = np.int16 if all(w.dtype == np.int16 for w in wavs) else np.float32
        wav, lens = _pack(wavs, wdtype)
        wav_dev = torch.from_numpy(wav).to(dev)
        if aligner is None:
            durs = [np.asarray(u["durations"], dtype=np.int64) for u in batch]
        else:
            durs = _aligned_durations(batch, wav_dev, lens, stft, aligner)
        feats = extract_features(wav_dev, lens, durs, stft=stft)
        f0s = [u.get("f0") for u in batch]
        if any(f is None for f in f0s):
            est = _f0_rows(wav_dev, lens, sampling_rate=pp["audio"]["sampling_rate"],
                           hop_length=pp["stft"]["hop_length"], method=f0_method, **f0_kw)
            f0s = [e if f is None else f for f, e in zip(f0s, est)]
        f0s = [np.asarray(f, dtype=np.float64) for f in f0s]
        ph = pitch_targets(f0s, durs, device=dev)
        pitches, energies = [], []
        for b, u in enumerate(batch):
            if ph[b] is None:  # preprocessor.py:264-265
                continue
            spk, name = u["speaker"], u["basename"]
            speakers.setdefault(spk, len(speakers))
            # frame level: the cropped contour as it is (the reference interpolates only before averaging)
            pitch = ph[b] if ph_pitch else f0s[b][:max(int(durs[b].sum()), 0)]
            energy = feats["energy"][b] if ph_energy else feats["energy_frame"][b]
            np.save(os.path.join(out_dir, "duration", f"{spk}-duration-{name}.npy"), durs[b])
            np.save(os.path.join(out_dir, "mel", f"{spk}-mel-{name}.npy"), feats["mel"][b])
            kept.append((spk, name, pitch, energy))
            pitches.append(pitch)
            energies.append(energy)
            lines.append("|".join([name, spk, "{" + " ".join(u["phones"]) + "}", u["raw_text"], u["aux"]]))
        pitch_stats.partial_fit(pitches)
        energy_stats.partial_fit(energies)

    batch = []
    for u in utterances:
        batch.append(u)
        if len(batch) == batch_size:
            flush(batch)
            batch = []
    if batch:
        flush(batch)

    p_mean, p_std = (pitch_stats.mean_, pitch_stats.scale_) if pp["pitch"]["normalization"] else (0, 1)
    e_mean, e_std = (energy_stats.mean_, energy_stats.scale_) if pp["energy"]["normalization"] else (0, 1)
    stats = {}
    for kind, idx, mean, std in (("pitch", 2, p_mean, p_std), ("energy", 3, e_mean, e_std)):
        values, vmin, vmax = normalize([k[idx] for k in kept], mean, std, device=dev)
        for k, v in zip(kept, values):
            np.save(os.path.join(out_dir, kind, f"{k[0]}-{kind}-{k[1]}.npy"), v)
        stats[kind] = [float(vmin), float(vmax), float(mean), float(std)]
    with open(os.path.join(out_dir, "speakers.json"), "w") as f:
        f.write(json.dumps(speakers))
    if emotions:
        with open(os.path.join(out_dir, "emotions.json"), "w") as f:
            f.write(json.dumps(emotions))
    with open(os.path.join(out_dir, "stats.json"), "w") as f:
        f.write(json.dumps(stats))
    random.Random(seed).shuffle(lines)
    with open(os.path.join(out_dir, "train.txt"), "w", encoding="utf-8") as f:
        for m in lines[val_size:]:
            f.write(m + "\n")
    with open(os.path.join(out_dir, "val.txt"), "w", encoding="utf-8") as f:
        for m in lines[:val_size]:
            f.write(m + "\n")
    return lines
