"""The yardstick of the inverse-audio tests: a float64 numpy restatement of STFT.transform,
STFT.inverse and griffin_lim (audio/stft.py:52-122, audio/audio_processing.py:66-82), one utterance
at a time, from the f32 bases, and the two parity statistics. test_audio_inv_host.py checks it
against the reference's own stored f32 outputs before test_gpu_audio_inv.py uses it."""
import os

import numpy as np

import _audio as A
from _npz_parts import load_npz_parts

N_FFT, HOP, N_BINS = A.N_FFT, A.HOP, A.N_BINS
GL_ITERS = 8                      # iterations of the stored Griffin-Lim results
WSUM_T = (1, 2, 3, 4, 5, 6, 71)   # frame counts of the stored window sums


def load_fixture():
    """audio_inv_a.npz beside audio_a.npz's utterances: per-utterance lists of the target
    magnitudes [513, T] (the reference's, from audio_a.npz), the initial angles, the reference's
    inverse and its 8-iteration Griffin-Lim signal (None for utterance 0, which has 3 frames)."""
    z = A.load_fixture()
    z.update(load_npz_parts(os.path.join(A.GOLDEN, "audio_inv_a.npz")))
    fr = z["frames"].astype(np.int64)
    z["mags"] = [np.ascontiguousarray(m.T) for m in z["ref_mag_list"]]
    off = np.concatenate([[0], np.cumsum(N_BINS * fr)])
    z["angles_list"] = [z["angles"][off[i]:off[i + 1]].reshape(N_BINS, fr[i]) for i in range(len(fr))]
    n = HOP * (fr - 1)
    off = np.concatenate([[0], np.cumsum(n)])
    z["ref_inverse_list"] = [z["ref_inverse"][off[i]:off[i + 1]] for i in range(len(fr))]
    off = np.concatenate([[0, 0], np.cumsum(n[1:])])
    z["ref_gl_list"] = [None] + [z["ref_gl"][off[i]:off[i + 1]] for i in range(1, len(fr))]
    z["ref_stats"] = {k: float(v) for k, v in zip(("W_inv", "W_inv_edge", "W_gl", "Z"), z["ref_stats"])}
    return z


def transform64(x, basis):
    """[1026, T] float64 spectrum (re rows, then im rows) of one utterance: reflect-pad by n_fft/2,
    hop, no clipping."""
    x = np.asarray(x, dtype=np.float64)
    p = np.pad(x, N_FFT // 2, mode="reflect")
    T = 1 + len(x) // HOP
    fr = p[np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]]
    return np.asarray(basis, dtype=np.float64).reshape(2 * N_BINS, N_FFT) @ fr.T


def project64(spec, mag):
    """mag * z / |z| per (bin, frame), and (mag, 0) where z = 0: what cos / sin of atan2(im, re) give."""
    re, im = np.asarray(spec[:N_BINS], dtype=np.float64), np.asarray(spec[N_BINS:], dtype=np.float64)
    mag = np.asarray(mag, dtype=np.float64)
    a = np.hypot(re, im)
    zero = a == 0
    a = np.where(zero, 1.0, a)
    return np.concatenate([np.where(zero, mag, mag * re / a), np.where(zero, 0.0, mag * im / a)])


def recombine64(mag, angles):
    mag, angles = np.asarray(mag, dtype=np.float64), np.asarray(angles, dtype=np.float64)
    return np.concatenate([mag * np.cos(angles), mag * np.sin(angles)])


def istft64(recomb, inverse_basis, wsum):
    """[256 (T - 1)] float64 signal of recomb [1026, T]: frames times the f32 inverse basis,
    overlap-add, division by the reference's f32 window sum (wsum, as data), times 4, trim."""
    recomb = np.asarray(recomb, dtype=np.float64)
    T = recomb.shape[1]
    y = recomb.T @ np.asarray(inverse_basis, dtype=np.float64).reshape(2 * N_BINS, N_FFT)
    ola = np.zeros(N_FFT + HOP * (T - 1))
    for t in range(T):
        ola[HOP * t:HOP * t + N_FFT] += y[t]
    assert wsum.shape == ola.shape and wsum.dtype == np.float32
    keep = slice(N_FFT // 2, len(ola) - N_FFT // 2)  # the window sum is at least 1.25 there (0 at sample 0)
    return ola[keep] / wsum[keep].astype(np.float64) * (N_FFT / HOP)


def gl64(mag, angles, n_iters, basis, inverse_basis, wsum, trace=None):
    """Griffin-Lim in float64 from the given initial angles. trace: a list that receives the
    spectral convergence || |STFT(signal)| - mag || / || mag || of the signal before each
    projection (index 0: of the initial inverse)."""
    sig = istft64(recombine64(mag, angles), inverse_basis, wsum)
    for _ in range(n_iters):
        spec = transform64(sig, basis)
        if trace is not None:
            trace.append(spectral_convergence(spec, mag))
        sig = istft64(project64(spec, mag), inverse_basis, wsum)
    return sig


def spectral_convergence(spec, mag):
    m = np.hypot(np.asarray(spec[:N_BINS], dtype=np.float64), np.asarray(spec[N_BINS:], dtype=np.float64))
    mag = np.asarray(mag, dtype=np.float64)
    return float(np.linalg.norm(m - mag) / np.linalg.norm(mag))


def stat_W(wav, wav64):
    """max |wav - wav64| / max |wav64|"""
    return float(np.abs(np.asarray(wav, dtype=np.float64) - wav64).max() / np.abs(wav64).max())


def stat_W_edge(wav, wav64):
    """W restricted to the first and the last 256 samples (the peak is still the whole signal's)."""
    d = np.abs(np.asarray(wav, dtype=np.float64) - wav64)
    return float(max(d[:HOP].max(), d[-HOP:].max()) / np.abs(wav64).max())


def stat_Z(spec, spec64):
    """max |spec - spec64|"""
    return float(np.abs(np.asarray(spec, dtype=np.float64) - spec64).max())
