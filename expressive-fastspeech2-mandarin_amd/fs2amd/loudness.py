"""Integrated loudness (ITU-R BS.1770-4 / EBU R128) and loudness normalisation of mono waveforms on the
GPU: K-weighting (``fs2amd.audio.k_weighting_sos``) through ``ops.sosfilt``, the two-stage gating of
``ops.loudness_gate`` and the gain of ``ops.gain_int16`` (include/fs2hip_iir.h). It is BS.1770's rule in
this project's own float64 arithmetic, not the bits of pyloudnorm or ffmpeg; one channel only. The
device takes no logarithm: the host turns the gated mean square into LUFS.

Below 44.1 kHz the bilinear K-weighting design is warped: a full-scale 997 Hz sine reads -3.01 LUFS at
48 kHz, -2.98 at 22.05 kHz and -2.97 at 16 kHz. That is the design every BS.1770 implementation at
those rates shares, and it is left as it is.
"""
import collections
import math

import numpy as np
import torch

ABS_GATE_LUFS = -70.0
REL_GATE_LU = -10.0
OFFSET = -0.691

LoudnessRecord = collections.namedtuple("LoudnessRecord", "lufs gain clipped unmeasured")


def full_scale(dtype):
    """32768 for int16 waveforms, 1 for float32 ones."""
    return 32768.0 if np.dtype(dtype) == np.int16 else 1.0


def gate_hop(sampling_rate):
    """The 100 ms hop of the 400 ms gating blocks in samples: round(fs / 10)."""
    return int(round(float(sampling_rate) / 10.0))


def abs_gate(dtype):
    """The absolute gate (-70 LUFS) as a mean square in the units of a waveform of ``dtype``."""
    return 10.0 ** ((ABS_GATE_LUFS - OFFSET) / 10.0) * full_scale(dtype) ** 2


def target_z(target_lufs, dtype):
    """The mean square that reads ``target_lufs``, in the units of a waveform of ``dtype``."""
    return 10.0 ** ((float(target_lufs) - OFFSET) / 10.0) * full_scale(dtype) ** 2


def lufs_of(zbar, dtype):
    """-0.691 + 10 log10(zbar / full_scale ** 2) on the host; -inf for an unmeasured row (zbar 0)."""
    z = float(zbar)
    return -math.inf if not z > 0.0 else OFFSET + 10.0 * math.log10(z / full_scale(dtype) ** 2)


class KWeighting:
    """The device tensors one sampling rate needs: sections, tables, hop."""

    def __init__(self, sampling_rate, device):
        from . import ops
        from .audio import k_weighting_sos

        self.sos = k_weighting_sos(sampling_rate)
        self.tables = torch.from_numpy(ops.sos_tables(self.sos)).to(device)
        self.hop = gate_hop(sampling_rate)


def measure_batch(wav_dev, lens_dev, kw):
    """LoudnessGateOut of an uploaded int16 / float32 batch: ops.sosfilt, then ops.loudness_gate."""
    from . import ops

    dtype = np.int16 if wav_dev.dtype == torch.int16 else np.float32
    y = ops.sosfilt(wav_dev, kw.sos, lens_dev, tables=kw.tables).y
    return ops.loudness_gate(y, lens_dev, hop=kw.hop, abs_gate=abs_gate(dtype), rel_factor=10.0 ** (REL_GATE_LU / 10.0))


def normalize_batch(wav_dev, lens_dev, kw, *, target_lufs, peak_ceiling=None):
    """(LoudnessGateOut, GainOut) of an uploaded batch: measured, then brought to target_lufs.
    peak_ceiling is in the waveform's own units."""
    from . import ops

    dtype = np.int16 if wav_dev.dtype == torch.int16 else np.float32
    g = measure_batch(wav_dev, lens_dev, kw)
    return g, ops.gain_int16(wav_dev, g.zbar, lens_dev, target_z=target_z(target_lufs, dtype), peak_ceiling=peak_ceiling)


def _groups(wavs):
    wavs = [np.asarray(w) for w in wavs]
    if any(w.ndim != 1 or w.dtype not in (np.int16, np.float32) for w in wavs):
        raise ValueError("fs2amd: waveforms are 1-D int16 or float32 arrays")
    for dtype in (np.int16, np.float32):
        idx = [b for b, w in enumerate(wavs) if w.dtype == dtype]
        if idx:
            yield dtype, idx, [wavs[b] for b in idx]


def integrated_loudness(wavs, *, sampling_rate, device=None):
    """The integrated loudness in LUFS of each of a list of 1-D mono waveforms, int16 (full scale 32768)
    or float32 (full scale 1.0): K-weighting, 400 ms blocks every 100 ms, the absolute gate at -70 LUFS
    and the relative gate 10 LU under the mean of what passed it. -inf for a waveform with no block
    above the gates (shorter than 400 ms, or silent). Each dtype is one batch on the device."""
    from .preprocess import _device, _pack

    dev = _device(device)
    kw = KWeighting(sampling_rate, dev)
    res = [None] * len(wavs)
    for dtype, idx, group in _groups(wavs):
        wav, lens = _pack(group, dtype)
        g = measure_batch(torch.from_numpy(wav).to(dev), torch.from_numpy(lens).to(dev), kw)
        for b, z in zip(idx, g.zbar.cpu().tolist()):
            res[b] = lufs_of(z, dtype)
    return res


def normalize_loudness(wavs, *, sampling_rate, target_lufs=-23.0, peak_ceiling=None, device=None):
    """Each of a list of 1-D mono waveforms brought to ``target_lufs`` by one gain per waveform. Returns
    (the waveforms in their own dtype, a LoudnessRecord(lufs, gain, clipped, unmeasured) per waveform):
    lufs is the measured loudness before the gain; int16 output is rounded to nearest and saturated,
    and ``clipped`` counts the saturated samples; float32 output is not saturated. peak_ceiling: None,
    or the largest |sample| allowed as a fraction of full scale (1.0 = full scale): the gain is lowered
    where it would exceed that, never raised. An unmeasured waveform (-inf LUFS) comes back unchanged."""
    from .preprocess import _device, _pack

    dev = _device(device)
    kw = KWeighting(sampling_rate, dev)
    out, recs = [None] * len(wavs), [None] * len(wavs)
    for dtype, idx, group in _groups(wavs):
        wav, lens = _pack(group, dtype)
        ceiling = None if peak_ceiling is None else float(peak_ceiling) * full_scale(dtype)
        g, r = normalize_batch(torch.from_numpy(wav).to(dev), torch.from_numpy(lens).to(dev), kw,
                               target_lufs=target_lufs, peak_ceiling=ceiling)
        q, zbar, gain = r.q.cpu().numpy(), g.zbar.cpu().tolist(), r.gain.cpu().tolist()
        clipped, unmeasured = r.clipped.cpu().tolist(), r.unmeasured.cpu().tolist()
        for j, b in enumerate(idx):
            out[b] = q[j, :int(lens[j])].copy()
            recs[b] = LoudnessRecord(lufs_of(zbar[j], dtype), gain[j], int(clipped[j]), bool(unmeasured[j]))
    return out, recs
