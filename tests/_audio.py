"""The yardstick of the audio tests: a float64 numpy restatement of TacotronSTFT.mel_spectrogram
(audio/stft.py:52-81,159-178 behind audio/tools.py:8-15), one utterance at a time, and the three
parity statistics. test_audio_host.py checks it against the reference's own stored f32 outputs
before test_gpu_audio.py uses it."""
import os

import numpy as np

from _npz_parts import load_npz_parts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_FFT, HOP, N_MEL, N_BINS, CLIP = 1024, 256, 80, 513, 1e-5


def load_fixture():
    z = load_npz_parts(os.path.join(GOLDEN, "audio_a.npz"))
    lens = z["lens"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    z["wavs"] = [z["samples"][off[i]:off[i + 1]] for i in range(len(lens))]
    fr = z["frames"].astype(np.int64)
    foff = np.concatenate([[0], np.cumsum(fr)])
    for k in ("ref_mel", "ref_energy", "ref_mag"):  # stored concatenated over frames
        z[k + "_list"] = [z[k][foff[i]:foff[i + 1]] for i in range(len(lens))]
    return z


def frames64(x, pad_mode="reflect"):
    """[T, n_fft] float64 frames of one utterance: clip, pad by n_fft/2, hop."""
    x = np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0)
    p = np.pad(x, N_FFT // 2, mode=pad_mode)
    T = 1 + len(x) // HOP
    return p[np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]]


def features64(x, basis, mel_basis, pad_mode="reflect"):
    """(mag [T, 513], linear mel [T, 80], energy [T]) in float64 from the f32 bases."""
    spec = frames64(x, pad_mode) @ np.asarray(basis, dtype=np.float64).reshape(2 * N_BINS, N_FFT).T
    mag = np.sqrt(spec[:, :N_BINS] ** 2 + spec[:, N_BINS:] ** 2)
    return mag, mag @ np.asarray(mel_basis, dtype=np.float64).T, np.sqrt((mag ** 2).sum(1))


def parity_stats(mel, energy, mel64_lin, e64, mag=None, mag64=None):
    """A, G, E (and M for the magnitudes) of an f32 result against the float64 restatement:
      A = max |exp(mel) - max(mel64_lin, 1e-5)|
      G = max |mel - log mel64_lin|   where mel64_lin >= 1e-3
      E = max |energy - e64| / max(e64, 1e-3)
      M = max |mag - mag64|"""
    mel, energy = np.asarray(mel, dtype=np.float64), np.asarray(energy, dtype=np.float64)
    A = np.abs(np.exp(mel) - np.maximum(mel64_lin, CLIP)).max()
    sel = mel64_lin >= 1e-3
    G = np.abs(mel[sel] - np.log(mel64_lin[sel])).max()
    E = (np.abs(energy - e64) / np.maximum(e64, 1e-3)).max()
    out = {"A": float(A), "G": float(G), "E": float(E)}
    if mag is not None:
        out["M"] = float(np.abs(np.asarray(mag, dtype=np.float64) - mag64).max())
    return out


def fixture_stats(z, basis):
    """Statistics of the reference's stored f32 outputs over the whole fixture, and the float64
    restatement per utterance: ({A, G, E, M}, [(mag64, mel64_lin, e64), ...]). basis: the f32
    forward basis (fs2amd.audio.stft_forward_basis; the fixture pins its bytes by hash)."""
    r64 = [features64(w, basis, z["mel_basis"]) for w in z["wavs"]]
    cat = [np.concatenate([r[i] for r in r64]) for i in range(3)]
    return parity_stats(z["ref_mel"], z["ref_energy"], cat[1], cat[2], z["ref_mag"], cat[0]), r64


def segment_mean_loop(energy, duration):
    """preprocessor/preprocessor.py:293-302, verbatim semantics: the in-place loop."""
    energy = np.array(energy, dtype=np.float32)
    pos = 0
    for i, d in enumerate(duration):
        energy[i] = np.mean(energy[pos:pos + d]) if d > 0 else 0
        pos += d
    return energy[:len(duration)]
