"""Training-target extraction on the GPU: the reference's ``audio/`` package (audio/stft.py:130-178
``TacotronSTFT``, audio/tools.py:8-15 ``get_mel_from_wav``) and the per-utterance feature code of
preprocessor/preprocessor.py:267-302, over ragged batches, as one fs2_mel_spectrogram launch
(include/fs2hip_audio.h; exact-f32 MFMA) plus one fs2_segment_mean launch.

    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to("cuda")
    mel, energy = get_mel_from_wav(wav_float_numpy, stft)        # [80, T], [T] numpy, as the reference
    feats = extract_features(wavs, lens, durations, stft=stft)    # a batch: what fs2amd.pipeline collates

GPU only, like the vocoder: CPU tensors raise. Out of scope here: pitch (WORLD), the inverse STFT /
Griffin-Lim, outlier removal and the normalisation statistics.
"""
import numpy as np
import torch

CLIP_VAL = 1e-5  # audio/audio_processing.py:85 dynamic_range_compression


def _hz_to_mel(f):
    """Slaney (Auditory Toolbox) mel scale: linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (np.maximum(m, min_log_mel) - min_log_mel)), f_sp * m)


def mel_band_edges(sr, n_mels, fmin, fmax):
    """The n_mels + 2 band edge frequencies (Hz, float64): equally spaced on the Slaney mel scale."""
    fmax = sr / 2.0 if fmax is None else fmax
    return _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel's default construction, restated: triangular filters whose edges are
    equally spaced on the Slaney mel scale (htk=False), each scaled to unit area over its band
    (norm="slaney": row i times 2 / (f[i+2] - f[i])), computed in float64 and cast to float32
    [n_mels, n_fft/2 + 1].

    librosa is not a dependency of this project and parity with it is not pinned by the tests;
    they pin the construction's properties instead (shape, support, single peak per row, centre
    spacing, area normalisation)."""
    f = mel_band_edges(sr, n_mels, fmin, fmax)
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    fdiff = np.diff(f)
    ramps = f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (f[2:] - f[:-2]))[:, None]
    return w.astype(np.float32)


def hann_periodic(n):
    """scipy.signal.get_window("hann", n, fftbins=True): float64."""
    fac = np.linspace(-np.pi, np.pi, n + 1)
    return (0.5 * np.cos(0.0 * fac) + 0.5 * np.cos(fac))[:-1]


def stft_forward_basis(filter_length, win_length=None):
    """The windowed Fourier basis of the reference's STFT.__init__ (audio/stft.py:26-49), f32
    [2 * (filter_length/2 + 1), 1, filter_length]: float64 FFT of the identity, real rows then
    imaginary rows, cast to f32, multiplied in f32 by the f32 periodic Hann window (centre-padded
    to filter_length)."""
    win_length = filter_length if win_length is None else win_length
    assert filter_length >= win_length
    fb = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    fb = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])
    basis = torch.from_numpy(fb[:, None, :]).to(torch.float32)
    win = np.zeros(filter_length)
    lpad = (filter_length - win_length) // 2
    win[lpad:lpad + win_length] = hann_periodic(win_length)
    basis *= torch.from_numpy(win).float()
    return basis


def n_frames(n_samples, hop_length=256, filter_length=1024):
    """Frames of an utterance of n_samples: 1 + n // hop (reflect padding by filter_length / 2 on
    both sides); 0 when n <= filter_length / 2, which cannot be reflect-padded (the reference
    raises there)."""
    return 1 + n_samples // hop_length if n_samples > filter_length // 2 else 0


class STFT(torch.nn.Module):
    """The forward half of the reference's STFT module: holds ``forward_basis``."""

    def __init__(self, filter_length, hop_length, win_length, window="hann"):
        super().__init__()
        if window != "hann":
            raise ValueError("fs2amd.audio: only the Hann window is built")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.register_buffer("forward_basis", stft_forward_basis(filter_length, win_length))


class TacotronSTFT(torch.nn.Module):
    """Drop-in for audio/stft.py:130-178. ``mel_spectrogram(y)`` returns (mel [B, n_mel, T], energy
    [B, T]) as the reference does (the mel is a transposed view of the kernel's channels-last
    result); ``lens=`` (samples per row) makes the batch ragged: every utterance is reflect-padded
    at its own ends and rows past its frame count are 0. Move it to the GPU with ``.to("cuda")``."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050,
                 mel_fmin=0.0, mel_fmax=8000.0, max_wav_value=32768.0):
        super().__init__()
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        self.max_wav_value, self.clip_val = float(max_wav_value), CLIP_VAL
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        self.register_buffer("mel_basis", torch.from_numpy(
            mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)))

    @property
    def forward_basis(self):
        return self.stft_fn.forward_basis

    def spectral_normalize(self, magnitudes):
        return torch.log(torch.clamp(magnitudes, min=self.clip_val))

    def spectral_de_normalize(self, magnitudes):
        return torch.exp(magnitudes)

    def mel_spectrogram(self, y, lens=None):
        from . import ops

        if not y.is_cuda:
            raise RuntimeError("fs2amd: TacotronSTFT runs on the HIP kernels only (no CPU fallback)")
        if y.dtype != torch.int16:
            # the reference's asserts; under a ragged batch only the samples below lens count
            v = y if lens is None else y.masked_fill(
                torch.arange(y.shape[1], device=y.device)[None, :] >= torch.as_tensor(lens, device=y.device)[:, None], 0)
            assert torch.min(v) >= -1
            assert torch.max(v) <= 1
        mel, energy, _ = ops.mel_spectrogram(y, lens, stft=self)
        return mel.transpose(1, 2), energy


def get_mel_from_wav(audio, _stft):
    """audio/tools.py:8-15: one utterance, numpy float samples in, (mel [n_mel, T], energy [T])
    float32 numpy out; samples are clipped to [-1, 1]."""
    from . import ops

    dev = _stft.mel_basis.device
    wav = torch.as_tensor(np.asarray(audio), dtype=torch.float32).reshape(1, -1).to(dev)
    mel, energy, _ = ops.mel_spectrogram(wav, None, stft=_stft)  # the kernel clips on load
    return mel[0].t().cpu().numpy().astype(np.float32), energy[0].cpu().numpy().astype(np.float32)


def extract_features(wavs, lens, durations=None, *, stft):
    """Mel / energy targets of a ragged batch, as preprocessor.py:267-302 computes them per
    utterance. wavs [B, n_max] f32 or int16 on the GPU, lens [B] samples, durations: None or a list
    of B integer arrays (frames per phoneme). Returns a dict of per-utterance numpy arrays, the
    shapes fs2amd.pipeline collates:

      "mel"            [T_b, n_mel]  cropped to sum(duration) frames when durations are given
      "energy_frame"   [T_b]
      "energy"         [L_b] phoneme-level means (only with durations; 0 where d = 0)
      "frames"         int64 [B], before the crop

    The lengths come back in one device->host copy (with the features). Durations are expected to
    fit their utterance (sum(d) <= frames), as the reference's aligner output does."""
    from . import ops

    B = wavs.shape[0]
    lens_t = torch.as_tensor(lens).to(torch.int64).cpu()
    mel, energy, frames = ops.mel_spectrogram(wavs, lens_t, stft=stft)
    ph = None
    if durations is not None:
        Lx = max(max(len(d) for d in durations), 1)
        dur = torch.zeros(B, Lx, dtype=torch.int64)
        for b, d in enumerate(durations):
            dur[b, :len(d)] = torch.as_tensor(np.asarray(d), dtype=torch.int64)
        ph = ops.segment_mean(energy, dur.to(wavs.device))
    packed = torch.cat([mel.reshape(B, -1), energy, frames.to(torch.float32)[:, None]] + ([ph] if ph is not None else []),
                       dim=1).cpu().numpy()  # one copy
    T, n_mel = mel.shape[1], mel.shape[2]
    out = {"mel": [], "energy_frame": [], "frames": packed[:, T * n_mel + T].astype(np.int64)}
    if ph is not None:
        out["energy"] = []
    for b in range(B):
        t = int(out["frames"][b])
        if durations is not None:
            t = min(t, int(np.sum(durations[b])))
        out["mel"].append(packed[b, :T * n_mel].reshape(T, n_mel)[:t].copy())
        out["energy_frame"].append(packed[b, T * n_mel:T * n_mel + T][:t].copy())
        if ph is not None:
            out["energy"].append(packed[b, T * n_mel + T + 1:][:len(durations[b])].copy())
    return out
