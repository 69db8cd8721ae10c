"""Audio feature extraction, host side (no GPU): the mel filterbank's construction, the Fourier basis
against the reference-built one, the frame count, the C ABI of include/fs2hip_audio.h, and the
float64 yardstick of test_gpu_audio.py against the reference's own stored outputs."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

import _audio as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_audio.h")
SR, N_FFT, N_MEL, FMIN, FMAX = 22050, 1024, 80, 0.0, 8000.0


@pytest.fixture(scope="module")
def fx():
    return A.load_fixture()


@pytest.fixture(scope="module")
def basis():
    from fs2amd.audio import stft_forward_basis

    return stft_forward_basis(N_FFT, N_FFT).numpy().reshape(2 * A.N_BINS, N_FFT)


def test_mel_filterbank_properties():
    from fs2amd.audio import mel_band_edges, mel_filterbank

    w = mel_filterbank(SR, N_FFT, N_MEL, FMIN, FMAX)
    assert w.shape == (80, 513) and w.dtype == np.float32
    assert (w >= 0).all()
    fft_f = np.linspace(0, SR / 2, 513)
    f = mel_band_edges(SR, N_MEL, FMIN, FMAX)
    assert f.shape == (82,) and f[0] == FMIN and abs(f[-1] - FMAX) < 1e-6
    for i in range(N_MEL):
        nz = np.nonzero(w[i])[0]
        assert len(nz) > 0, i  # no empty band at this resolution
        # support inside the band's own edges, hence inside [fmin, fmax]
        assert fft_f[nz[0]] > f[i] - 1e-9 and fft_f[nz[-1]] < f[i + 2] + 1e-9, i
        # a single peak: rises to it, falls after it
        p = int(np.argmax(w[i]))
        d = np.diff(w[i].astype(np.float64))
        assert (d[:p] >= 0).all() and (d[p:] <= 0).all(), i
        assert abs(fft_f[p] - f[i + 1]) <= SR / N_FFT, i  # the peak is the bin nearest the centre
    assert not w[:, fft_f > FMAX].any()
    # centre spacing: linear (200/3 Hz per mel) below 1 kHz, logarithmic (6.4 ** (1/27) per mel) above
    c = f[1:-1]
    step = (A_hz_to_mel(FMAX) - A_hz_to_mel(FMIN)) / (N_MEL + 1)
    lin = c[c < 1000.0]
    assert len(lin) > 10 and np.allclose(np.diff(lin), step * 200.0 / 3, rtol=1e-9)
    log = c[c >= 1000.0]
    assert len(log) > 10 and np.allclose(log[1:] / log[:-1], 6.4 ** (step / 27.0), rtol=1e-9)
    # Slaney area normalisation: row i is the unit-height triangle times 2 / (f[i+2] - f[i])
    for i in (0, 17, 40, 79):
        lower = (fft_f - f[i]) / (f[i + 1] - f[i])
        upper = (f[i + 2] - fft_f) / (f[i + 2] - f[i + 1])
        tri = np.maximum(0, np.minimum(lower, upper))
        np.testing.assert_allclose(w[i], (tri * 2.0 / (f[i + 2] - f[i])).astype(np.float32), rtol=1e-6, atol=0)


def A_hz_to_mel(f):
    """Slaney scale written out independently of fs2amd.audio."""
    return f / (200.0 / 3) if f < 1000.0 else 15.0 + np.log(f / 1000.0) / (np.log(6.4) / 27.0)


def test_forward_basis_is_the_reference_built_one_bit_for_bit(fx, basis):
    assert basis.dtype == np.float32 and basis.shape == (1026, 1024)
    ids = fx["basis_row_ids"]
    np.testing.assert_array_equal(basis[ids], fx["basis_rows"])  # readable failure first
    digest = hashlib.sha256(basis.astype("<f4").tobytes()).digest()
    assert digest == fx["basis_sha256"].tobytes()  # every bit of all 1026 x 1024 values
    from fs2amd.audio import TacotronSTFT

    t = TacotronSTFT(1024, 256, 1024, 80, SR, FMIN, FMAX)
    assert t.stft_fn.forward_basis.shape == (1026, 1, 1024)
    assert set(t.state_dict()) == {"stft_fn.forward_basis", "mel_basis"}
    np.testing.assert_array_equal(t.mel_basis.numpy(), fx["mel_basis"])


def test_frame_count_formula(fx):
    from fs2amd import ops
    from fs2amd.audio import n_frames

    assert [n_frames(int(n)) for n in fx["lens"]] == list(fx["frames"]) == [3, 5, 5, 34, 71]
    assert [n_frames(n) for n in (0, 1, 512, 513, 767, 768)] == [0, 0, 0, 3, 3, 4]
    lens = torch.tensor([0, 512, 513, 1024, 17921])
    assert ops.mel_frames(lens).tolist() == [0, 0, 3, 5, 71]
    for w, fr in zip(fx["wavs"], fx["frames"]):
        assert A.frames64(w).shape == (fr, 1024)


def test_audio_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_AUDIO) == ["fs2_mel_spectrogram", "fs2_segment_mean"], declared
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY))
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_AUDIO[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_audio.h" in _lib.EXTRA_HEADERS  # the build id covers the header
    assert _lib.FS2_I16 == 3 and (_lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_FP8) == (0, 1, 2)


def test_mel_desc_layout_matches_header(tmp_path):
    from fs2amd import _lib

    names = [f[0] for f in _lib.MelDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fs2hip_audio.h"\nint main(void){' + "".join(
        f'printf("{n} %zu\\n", offsetof(fs2_mel_desc, {n}));' for n in names) + \
        'printf("size %zu\\n", sizeof(fs2_mel_desc)); printf("i16 %d\\n", FS2_I16); }\n'
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")],
                   check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert got.pop("size") == ctypes.sizeof(_lib.MelDesc) and got.pop("i16") == _lib.FS2_I16
    assert got == {n: getattr(_lib.MelDesc, n).offset for n in names}


def test_mel_entry_rejects_bad_descriptors_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    d = _lib.MelDesc()
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EINVAL
    for k in ("wav", "basis", "mel_basis", "mel", "energy"):
        setattr(d, k, 4096)
    d.B, d.n_max, d.T_out, d.wav_row_stride, d.clip_val = 2, 1024, 5, 1024, 1e-5
    d.n_fft, d.hop, d.win, d.n_mel = 512, 256, 512, 80
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EUNSUPPORTED
    d.n_fft, d.win, d.n_mel = 1024, 1024, 128
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EUNSUPPORTED
    d.n_mel, d.T_out = 80, 4  # lens NULL: every row has 1 + 1024 / 256 = 5 frames
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EINVAL
    host = (ctypes.c_int64 * 2)(513, 1279)
    d.lens, d.lens_host = 4096, ctypes.cast(host, ctypes.c_void_p)  # frames 3 and 5
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EINVAL
    d.T_out, d.wav_row_stride = 5, 1000
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EINVAL
    d.wav_row_stride, d.wav_dtype = 1024, _lib.FS2_BF16
    assert lib.fs2_mel_spectrogram(ctypes.byref(d), None) == _lib.FS2_EINVAL
    assert lib.fs2_segment_mean(None, None, 1, 1, 1, None, None) == _lib.FS2_EINVAL


def test_float64_yardstick_agrees_with_the_reference_outputs(fx, basis):
    """The restatement the GPU test measures against is the reference's computation: its stored f32
    magnitudes, energies and log-mels agree with it to f32 rounding (the figures of the issue's
    probe: ~1e-6 in linear mel, ~1e-4 in log-mel away from the clamp)."""
    stats, r64 = A.fixture_stats(fx, basis)
    print("reference vs float64:", stats)
    assert stats["A"] < 1e-5 and stats["G"] < 2e-4 and stats["E"] < 1e-5 and stats["M"] < 5e-4, stats
    assert [r[0].shape[0] for r in r64] == list(fx["frames"])
    # the fixture has what the exact GPU checks need: a frame of digital silence, and the clamp
    assert (fx["ref_mag"] == 0).all(axis=1).any()
    silent = (fx["ref_mag"] == 0).all(axis=1)
    assert (fx["ref_mel"][silent] == np.float32(np.log(np.float32(1e-5)))).all() and (fx["ref_energy"][silent] == 0).all()
    # reflection, not zero padding: the last frame would move by orders of magnitude more than any bound
    for i in range(1, 5):
        _, mz, _ = A.features64(fx["wavs"][i], basis, fx["mel_basis"], pad_mode="constant")
        assert np.abs(mz[-1] - r64[i][1][-1]).max() > 100 * 16 * stats["A"]


def test_segment_mean_fixture_is_the_plain_mean(fx):
    """The stored in-place loop results equal plain per-segment means, because the durations
    satisfy sum(d[:i]) >= i (include/fs2hip_audio.h)."""
    off = np.concatenate([[0], np.cumsum(fx["frames"])])
    for b, n in enumerate(fx["dur_lens"]):
        d = fx["dur"][b, :n]
        assert (d == 0).any() and all(d[:i].sum() >= i for i in range(n)) and d.sum() <= fx["frames"][b]
        e = fx["ref_energy"][off[b]:off[b + 1]]
        pos = np.concatenate([[0], np.cumsum(d)])
        plain = [e[pos[i]:pos[i + 1]].mean() if d[i] > 0 else 0.0 for i in range(n)]
        np.testing.assert_allclose(fx["ph_energy"][b, :n], plain, rtol=1e-6)
        np.testing.assert_array_equal(A.segment_mean_loop(e, d), fx["ph_energy"][b, :n])


def test_audio_api_is_exported_and_refuses_cpu_tensors():
    import fs2amd

    for name in ("TacotronSTFT", "get_mel_from_wav", "extract_features", "mel_filterbank"):
        assert hasattr(fs2amd, name) and name in fs2amd.__all__
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, SR, FMIN, FMAX)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft.mel_spectrogram(torch.zeros(1, 2048))
    x = torch.rand(3, 7)
    assert torch.equal(stft.spectral_de_normalize(stft.spectral_normalize(x + 1)), torch.exp(torch.log(x + 1)))
    import fs2amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        wav = torch.empty(3, 5000, device="cuda")
        mel, en, fr = torch.ops.fs2.mel_spectrogram(wav, None, torch.empty(1026, 1, 1024, device="cuda"),
                                                    torch.empty(80, 513, device="cuda"), 20, 256, 1024, 32768.0, 1e-5)
        assert mel.shape == (3, 20, 80) and en.shape == (3, 20) and fr.shape == (3,) and fr.dtype == torch.int64
