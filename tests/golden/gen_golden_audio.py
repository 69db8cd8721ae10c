#!/usr/bin/env python3
"""Generate tests/golden/audio_a.npz by running the REFERENCE's audio/stft.py on the CPU.

Runs only where the reference tree is mounted (FS2_REFERENCE, default /root/reference); only the
.npz travels. Two local accommodations let audio/stft.py and audio/tools.py import and run here:

* ``librosa`` is not installed: stand-in modules are put in ``sys.modules`` with the four names the
  reference uses: ``librosa.util.pad_center`` / ``tiny`` / ``normalize`` and ``librosa.filters.mel``.
  The mel stand-in calls THIS project's ``fs2amd.audio.mel_filterbank``. So the fixture's STFT
  magnitudes and energies are the reference's own (its basis, its reflect padding, its conv1d, its
  sqrt and norm), while the mel rows are the reference's matmul and log over this project's
  filterbank (stored as ``mel_basis``).
* audio/stft.py:68-72 calls ``.cuda()`` unconditionally: ``torch.Tensor.cuda`` is replaced by the
  identity for the duration of the script.

Five utterances, each run alone through the reference's ``get_mel_from_wav`` (clip, then
``TacotronSTFT.mel_spectrogram``), stored ragged (concatenated samples + ``lens``; outputs
concatenated over frames + ``frames``). The 4.2 MB forward basis is not stored: its sha256 is
(``basis_sha256``, over the little-endian f32 bytes), which pins every bit, with a few rows
(``basis_rows`` of ``basis_row_ids``) for a readable failure.

The phoneme-level energy (``ph_energy``) is the in-place loop of preprocessor/preprocessor.py:293-302
restated in tests/_audio.py (it sits inside Preprocessor.process_utterance, behind pyworld and tgt,
and cannot be called alone), run on the reference's energies.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_audio.py
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FS2_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.dirname(HERE))

from fs2amd.audio import mel_filterbank  # noqa: E402

import _audio as A  # noqa: E402
from _npz_parts import save_npz_parts  # noqa: E402

LENS = [513, 1024, 1279, 8548, 17921]
FRAMES = [3, 5, 5, 34, 71]
SR, FMIN, FMAX = 22050, 0, 8000
K_MAX = 16  # the widest parity factor the tests may use


def install_librosa_stand_ins():
    def pad_center(data, size=None, **kw):
        lpad = (size - len(data)) // 2
        return np.pad(data, (lpad, size - len(data) - lpad))

    def tiny(x):
        return np.finfo(np.asarray(x).dtype if np.issubdtype(np.asarray(x).dtype, np.floating) else np.float32).tiny

    def normalize(s, norm=None, **kw):
        assert norm is None
        return s

    lib, util, filters = types.ModuleType("librosa"), types.ModuleType("librosa.util"), types.ModuleType("librosa.filters")
    util.pad_center, util.tiny, util.normalize = pad_center, tiny, normalize
    filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    lib.util, lib.filters, lib.__path__ = util, filters, []
    sys.modules.update({"librosa": lib, "librosa.util": util, "librosa.filters": filters})


def import_reference_audio():
    install_librosa_stand_ins()
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import audio.stft as ref_stft
    import audio.tools as ref_tools
    assert ref_stft.__file__.startswith(REF)
    return ref_stft, ref_tools


def make_signal(n, rng, loud_tail=True):
    """Chirp + noise under a decaying envelope, loud within 512 samples of both ends."""
    t = np.arange(n) / SR
    f0, f1 = rng.uniform(80, 300), rng.uniform(2000, 7000)
    phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / max(t[-1], 1e-3) * t * t)
    env = 0.02 + 0.9 * np.exp(-3.0 * np.arange(n) / n)
    x = env * (np.sin(phase) + 0.3 * rng.standard_normal(n))
    x[-300:] += 0.7 * np.sin(2 * np.pi * 1234.0 * t[-300:]) * np.linspace(0.2, 1.0, 300)  # loud at the end
    x[:200] += 0.5 * np.sin(2 * np.pi * 777.0 * t[:200])  # and at the start
    return x


def main():
    ref_stft, ref_tools = import_reference_audio()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        stft = ref_stft.TacotronSTFT(1024, 256, 1024, 80, SR, FMIN, FMAX)
        rng = np.random.default_rng(20260)
        wavs = []
        for i, n in enumerate(LENS):
            x = make_signal(n, rng)
            if i >= 2:
                x[n // 3:n // 3 + 150] *= 2.5  # beyond +-1 before the clip
            if i == 4:
                x[9000:9000 + 2304] = 0.0  # digital silence: at least one whole frame
            wavs.append(x.astype(np.float32))
        assert any(np.abs(w).max() > 1.0 for w in wavs)
        for w in wavs:
            assert np.abs(w[:512]).max() > 0.3 and np.abs(w[-512:]).max() > 0.3
        mels, energies, mags = [], [], []
        for w, fr in zip(wavs, FRAMES):
            mel, energy = ref_tools.get_mel_from_wav(w, stft)  # [80, T], [T]
            mag, _ = stft.stft_fn.transform(torch.clip(torch.FloatTensor(w).unsqueeze(0), -1, 1))
            assert mel.shape == (80, fr) and energy.shape == (fr,) and mag.shape == (1, 513, fr)
            mels.append(np.ascontiguousarray(mel.T))
            energies.append(energy)
            mags.append(np.ascontiguousarray(mag[0].numpy().T))
        basis = stft.stft_fn.forward_basis.numpy().reshape(1026, 1024)
        mel_basis = stft.mel_basis.numpy()
    finally:
        torch.Tensor.cuda = real_cuda

    ref_mag = np.concatenate(mags)
    assert (ref_mag == 0).all(axis=1).any(), "no frame of digital silence"

    # the yardstick against the reference, and what a wrong padding would do to the last frame
    z = {"wavs": wavs, "mel_basis": mel_basis, "ref_mel": np.concatenate(mels), "ref_energy": np.concatenate(energies),
         "ref_mag": ref_mag}
    ref_stats, r64 = A.fixture_stats(z, basis)
    print("reference f32 vs float64 restatement:", ref_stats)
    for i in range(1, 5):
        _, mel_zero, _ = A.features64(wavs[i], basis, mel_basis, pad_mode="constant")
        moved = np.abs(np.maximum(mel_zero[-1], A.CLIP) - np.maximum(r64[i][1][-1], A.CLIP)).max()
        print(f"utterance {i}: zero padding moves the last frame's linear mel by {moved:.3e} "
              f"({moved / (K_MAX * ref_stats['A']):.0f}x the widest bound)")
        assert moved > 100 * K_MAX * ref_stats["A"], (i, moved)

    # durations: integers with zeros, sum(d[:i]) >= i, sum(d) <= frames
    durs = [[2, 0, 1], [2, 1, 0, 2], [3, 0, 0, 2]]
    for fr in FRAMES[3:]:
        while True:
            d = rng.integers(0, 6, size=fr // 3)
            d[0] = max(d[0], 2)
            if d.sum() <= fr and (d == 0).any() and all(d[:i].sum() >= i for i in range(len(d))):
                break
        durs.append(d.tolist())
    Lmax = max(len(d) for d in durs)
    dur = np.zeros((len(durs), Lmax), dtype=np.int64)
    ph = np.zeros((len(durs), Lmax), dtype=np.float32)
    for b, d in enumerate(durs):
        assert all(sum(d[:i]) >= i for i in range(len(d))) and 0 in d and sum(d) <= FRAMES[b]
        dur[b, :len(d)] = d
        ph[b, :len(d)] = A.segment_mean_loop(energies[b], d)

    rows = np.array([0, 1, 37, 255, 512, 513, 514, 700, 1025])
    n = save_npz_parts(
        os.path.join(HERE, "audio_a.npz"), samples=np.concatenate(wavs), lens=np.array(LENS, dtype=np.int64),
        frames=np.array(FRAMES, dtype=np.int64), mel_basis=mel_basis, ref_mel=z["ref_mel"], ref_energy=z["ref_energy"],
        ref_mag=ref_mag, basis_sha256=np.frombuffer(hashlib.sha256(basis.astype("<f4").tobytes()).digest(), dtype=np.uint8),
        basis_row_ids=rows, basis_rows=basis[rows], dur=dur, dur_lens=np.array([len(d) for d in durs], dtype=np.int64),
        ph_energy=ph)
    print("wrote audio_a.npz in", n, "part(s)")


if __name__ == "__main__":
    main()
