"""The reference's ``audio/`` package on the GPU, over ragged batches.

Forward (include/fs2hip_audio.h): audio/stft.py:130-178 ``TacotronSTFT``, audio/tools.py:8-15
``get_mel_from_wav`` and the per-utterance feature code of preprocessor/preprocessor.py:267-302, as
one fs2_mel_spectrogram launch (exact-f32 MFMA) plus one fs2_segment_mean launch.

    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to("cuda")
    mel, energy = get_mel_from_wav(wav_float_numpy, stft)        # [80, T], [T] numpy, as the reference
    feats = extract_features(wavs, lens, durations, stft=stft)    # a batch: what fs2amd.pipeline collates

Inverse (include/fs2hip_audio_inv.h): ``STFT.transform`` / ``inverse`` / ``forward``
(audio/stft.py:52-127), ``window_sumsquare`` and ``griffin_lim`` (audio/audio_processing.py:7-82) and
``inv_mel_spec`` (audio/tools.py:18-34): a mel-spectrogram to a waveform without a vocoder
checkpoint. A Griffin-Lim iteration is one fs2_stft launch (spectrum and projection onto the target
magnitudes) and one fs2_istft launch (overlap-add as a gather), both exact f32.

    audio = inv_mel_spec(mel_80xT, None, stft, griffin_iters=60)  # float32 samples, one utterance
    wav, lens = mel_to_wav(mel_BxTx80, mel_lens, stft)            # a ragged batch, the model's layout

GPU only, like the vocoder: CPU tensors raise. Out of scope here: pitch (WORLD), outlier removal and
the normalisation statistics.
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


def stft_inverse_basis(filter_length, hop_length, win_length=None):
    """The inverse basis of the reference's STFT.__init__ (audio/stft.py:34-47), f32
    [2 * (filter_length/2 + 1), 1, filter_length], built as the reference builds it: the float64
    pseudo-inverse of (filter_length / hop_length) times the stacked Fourier basis, transposed, cast
    to f32, multiplied in f32 by the f32 window. (The closed form agrees with the pinv to 3e-16 and
    still differs in about 1 % of the f32 bit patterns after the cast.)"""
    win_length = filter_length if win_length is None else win_length
    assert filter_length >= win_length
    scale = filter_length / hop_length
    fb = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    fb = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])
    inv = torch.from_numpy(np.linalg.pinv(scale * fb).T[:, None, :]).to(torch.float32)
    win = np.zeros(filter_length)
    lpad = (filter_length - win_length) // 2
    win[lpad:lpad + win_length] = hann_periodic(win_length)
    inv *= torch.from_numpy(win).float()
    return inv


def pack_inverse_basis(inverse_basis, hop_length=256):
    """The order fs2_istft's lanes read (include/fs2hip_audio_inv.h): f32 [129, 4, hop, 2, 4] with
    element (g, q, r, h, e) = inverse_basis[8g + 2e + h, hop * q + r]; the 1026 channels are padded
    with zero rows to 1032."""
    inv = inverse_basis.reshape(inverse_basis.shape[0], inverse_basis.shape[-1])
    C, n_fft = inv.shape
    kpad = (C + 7) // 8 * 8
    p = torch.zeros(kpad, n_fft, dtype=torch.float32)
    p[:C] = inv
    p = p.reshape(kpad // 8, 4, 2, n_fft // hop_length, hop_length)  # g, e, h, q, r
    return p.permute(0, 3, 4, 2, 1).contiguous()


def window_sumsquare(window, n_frames, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32, norm=None):
    """audio/audio_processing.py:7-63 (librosa 0.6): the sum-square envelope of the window at the
    hop length, [n_fft + hop_length * (n_frames - 1)]. The accumulator has `dtype`, the addends
    are float64 and the frames are added in ascending order, as in the reference's loop."""
    if window != "hann" or norm is not None:
        raise ValueError("fs2amd.audio: only the Hann window without normalisation is built")
    win_length = n_fft if win_length is None else win_length
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    win_sq = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    win_sq[lpad:lpad + win_length] = hann_periodic(win_length) ** 2
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


def wsum_edge_table(hop_length=256, win_length=1024, n_fft=1024):
    """window_sumsquare for fs2_istft, f32 [2 ** (n_fft / hop), hop]: position hop * j + r receives
    the frames j - q, q = 0 .. n_fft / hop - 1, that exist; row `mask` (bit q set = frame j - q
    exists) holds the f32 accumulator after adding win_sq[hop * q + r] for the set bits in
    ascending frame order (descending q), float64 addends, exactly as window_sumsquare's loop."""
    nq = n_fft // hop_length
    win_sq = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    win_sq[lpad:lpad + win_length] = hann_periodic(win_length) ** 2
    table = np.zeros((1 << nq, hop_length), dtype=np.float32)
    for mask in range(1 << nq):
        for q in reversed(range(nq)):
            if mask >> q & 1:
                table[mask] += win_sq[hop_length * q:hop_length * (q + 1)]
    return table


def window_sum_from_table(table, n_frames, hop_length=256, n_fft=1024):
    """window_sumsquare(n_frames) looked up in wsum_edge_table as the kernel does."""
    nq = n_fft // hop_length
    j = np.arange(n_frames - 1 + nq)
    mask = sum(((j - q >= 0) & (j - q < n_frames)).astype(np.int64) << q for q in range(nq))
    return table[mask].reshape(-1)


_INVERSE_BUFFERS = ("inverse_basis", "inverse_packed", "wsum_table")


class STFT(torch.nn.Module):
    """Drop-in for audio/stft.py:15-127. ``forward_basis`` is the module's only persistent buffer;
    ``inverse_basis`` [1026, 1, 1024] (and the two tables fs2_istft reads, ``inverse_packed`` and
    ``wsum_table``) are non-persistent buffers built on first use (the pseudo-inverse is about a
    second of SVD), on the device ``forward_basis`` is on. ``lens=`` / ``frames=`` make a batch
    ragged."""

    def __init__(self, filter_length, hop_length, win_length, window="hann"):
        super().__init__()
        if window != "hann":
            raise ValueError("fs2amd.audio: only the Hann window is built")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.register_buffer("forward_basis", stft_forward_basis(filter_length, win_length))

    def __getattr__(self, name):
        d = self.__dict__
        if name in _INVERSE_BUFFERS and name not in d.get("_buffers", {}) and not d.get("_building_inverse"):
            d["_building_inverse"] = True  # register_buffer asks hasattr(self, name)
            dev = self.forward_basis.device
            inv = stft_inverse_basis(self.filter_length, self.hop_length, self.win_length)
            self.register_buffer("inverse_basis", inv.to(dev), persistent=False)
            self.register_buffer("inverse_packed", pack_inverse_basis(inv, self.hop_length).to(dev), persistent=False)
            self.register_buffer("wsum_table", torch.from_numpy(
                wsum_edge_table(self.hop_length, self.win_length, self.filter_length)).to(dev), persistent=False)
            d["_building_inverse"] = False
        return super().__getattr__(name)

    def transform(self, input_data, lens=None):
        """(magnitude, phase), each [B, 513, T]: the kernel's spectrum, and torch.atan2 of it."""
        from . import ops

        out = ops.stft(input_data, lens, stft=self, want=("spec", "mag"))
        cutoff = self.filter_length // 2 + 1
        return out.mag, torch.atan2(out.spec[:, cutoff:], out.spec[:, :cutoff])

    def inverse(self, magnitude, phase, frames=None):
        """[B, 1, 256 (T - 1)] from magnitude and phase [B, 513, T]; the recombination is torch."""
        from . import ops

        recomb = torch.cat([magnitude * torch.cos(phase), magnitude * torch.sin(phase)], dim=1)
        n_out = self.hop_length * max(magnitude.shape[-1] - 1, 0)
        if n_out == 0:  # one frame: the reference's trim leaves no sample
            return magnitude.new_zeros(magnitude.shape[0], 1, 0)
        wav, _ = ops.istft(recomb, frames, stft=self, n_out_max=n_out)
        return wav[:, None, :]

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)


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


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None, frames=None, generator=None):
    """audio/audio_processing.py:66-82: magnitudes [B, 513, T] -> signal [B, 256 (T - 1)], on the GPU
    (fs2amd.ops.griffin_lim). angles: the initial phases [B, 513, T]; None draws them on the device
    (same distribution as the reference's np.random.rand, not its bits). frames: frames per
    utterance of a ragged batch; samples past 256 (frames - 1) are 0. Needs at least 4 frames per
    utterance, as the reference's reflect padding does: ValueError below that."""
    from . import ops

    wav, _ = ops.griffin_lim(magnitudes, frames, stft=stft_fn, n_iters=n_iters, angles=angles, generator=generator)
    return wav


def spec_from_mel(mel, _stft):
    """audio/tools.py:19-25: mel [n_mel, T] log-mel -> [1, 513, T] linear magnitudes, exp(mel) times
    the mel basis times 1000, on the host in the reference's arithmetic."""
    mel = torch.stack([torch.as_tensor(mel)])
    mel_decompress = _stft.spectral_de_normalize(mel).transpose(1, 2).data.cpu()
    out = torch.mm(mel_decompress[0], _stft.mel_basis.cpu())
    return out.transpose(0, 1).unsqueeze(0) * 1000


def write_wav_f32(path, sampling_rate, audio):
    """A mono IEEE-float WAV file, as scipy.io.wavfile.write gives for float32 samples."""
    import struct

    data = np.ascontiguousarray(audio, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, sampling_rate, sampling_rate * 4, 4, 32)
    fact = struct.pack("<I", len(data) // 4)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<I", 4) + fact + \
        b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def inv_mel_spec(mel, out_filename, _stft, griffin_iters=60, angles=None):
    """audio/tools.py:18-34: mel [n_mel, T] -> Griffin-Lim audio of its first T - 1 frames (the
    reference drops the last one), written to out_filename as a float32 WAV at
    _stft.sampling_rate and returned as float32 numpy samples; out_filename None only returns
    them. Uses ``_stft.stft_fn`` (the reference's ``_stft._stft_fn`` raises AttributeError)."""
    dev = _stft.mel_basis.device
    if dev.type != "cuda":
        raise RuntimeError("fs2amd: inv_mel_spec runs on the HIP kernels only (no CPU fallback)")
    spec = spec_from_mel(mel, _stft)[:, :, :-1].contiguous().to(dev)
    audio = griffin_lim(spec, _stft.stft_fn, griffin_iters, angles=angles)
    audio = audio.squeeze().cpu().numpy().astype(np.float32)
    if out_filename is not None:
        write_wav_f32(out_filename, _stft.sampling_rate, audio)
    return audio


def mel_to_wav(mel, mel_lens, stft, n_iters=60, angles=None):
    """inv_mel_spec for a ragged batch in the model's output layout: mel [B, T, n_mel] log-mel,
    mel_lens [B] frames -> (wav f32 [B, 256 (T - 2)] on the GPU, lens int64 numpy [B] = 256 *
    (mel_lens - 2)): every utterance gets what inv_mel_spec gives for mel[b, :mel_lens[b]].T from
    the same initial angles ([B, 513, T - 1]). Needs mel_lens >= 5."""
    lens = torch.as_tensor(mel_lens).to(torch.int64).cpu()
    B, T = mel.shape[0], mel.shape[1]
    if lens.shape != (B,) or int(lens.max()) > T:
        raise ValueError(f"fs2amd: mel_lens must be [{B}] frame counts of at most {T}")
    frames = lens - 1
    if int(frames.min()) < 4:
        raise ValueError("fs2amd: griffin_lim needs at least 4 frames per utterance (mel_lens >= 5)")
    dev = stft.mel_basis.device
    if dev.type != "cuda":
        raise RuntimeError("fs2amd: mel_to_wav runs on the HIP kernels only (no CPU fallback)")
    n_bins = stft.mel_basis.shape[1]
    mag = torch.zeros(B, n_bins, T - 1)
    for b in range(B):
        mag[b, :, :frames[b]] = spec_from_mel(mel[b, :lens[b]].t(), stft)[0, :, :-1]
    from . import ops

    wav, _ = ops.griffin_lim(mag.to(dev), frames, stft=stft, n_iters=n_iters, angles=angles)
    return wav, (stft.hop_length * (frames - 1)).numpy()


def resample_ratio(target_rate, source_rate):
    """(up, down) of include/fs2hip_resample.h: target / g and source / g with g their gcd."""
    import math

    target_rate, source_rate = int(target_rate), int(source_rate)
    if target_rate < 1 or source_rate < 1:
        raise ValueError(f"fs2amd: sampling rates must be positive integers, got {source_rate} -> {target_rate}")
    g = math.gcd(target_rate, source_rate)
    return target_rate // g, source_rate // g


def resample_taps(up, down, beta=5.0):
    """The low-pass of scipy.signal.resample_poly's default design, float64, in numpy alone: with
    half = 10 * max(up, down) and c = 1 / max(up, down), the 2 * half + 1 taps
    c * sinc(c * (k - half)) * kaiser(beta), divided by their sum (include/fs2hip_resample.h).
    The kernel takes ``resample_taps(up, down) * up``. np.kaiser and scipy's window use different
    fits of i0, so the taps are scipy's firwin to a few 1e-16 of the largest tap, not bit for bit."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"fs2amd: resample_taps needs up, down >= 1, got {up}, {down}")
    half = 10 * max(up, down)
    c = 1.0 / max(up, down)
    h = c * np.sinc(c * (np.arange(2 * half + 1, dtype=np.float64) - half)) * np.kaiser(2 * half + 1, float(beta))
    return h / h.sum()


def k_weighting_sos(sampling_rate):
    """The K-weighting of ITU-R BS.1770 at ``sampling_rate`` as float64 [2, 6] second-order sections in
    scipy's layout (b0 b1 b2 1 a1 a2): the high shelf, then the high-pass. The standard tabulates the
    coefficients at 48 kHz only; this is De Man's bilinear design of the two analogue prototypes, which
    reproduces that table to all its published digits. With K = tan(pi * f0 / fs) and
    a0 = 1 + K / Q + K * K, a = [1, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0] for both;
    the shelf has b = [(Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
    the high-pass b = [1, -2, 1]. The bilinear transform warps the shelf as the rate falls: a
    full-scale 997 Hz sine reads -3.01 LUFS at 48 kHz and about -2.97 at 16 kHz."""
    import math

    fs = float(sampling_rate)
    if not fs > 0.0 or not math.isfinite(fs):
        raise ValueError(f"fs2amd: k_weighting_sos needs a positive sampling rate, got {sampling_rate!r}")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    if not fs > 2.0 * f0:
        raise ValueError(f"fs2amd: k_weighting_sos needs a sampling rate above {2 * f0:.0f} Hz, got {sampling_rate!r}")
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], dtype=np.float64)


SOS_BLOCK, SOS_TABLE_LEN = 64, 412  # FS2_IIR_BLOCK, FS2_IIR_TABLE_LEN of include/fs2hip_iir.h


def sos_tables(sos):
    """The per-section tables fs2_sosfilt takes (include/fs2hip_iir.h, rule 3), float64 [S, 412], computed
    in plain Python floats (IEEE double, one rounding per operation, in the header's order): the zero-input
    responses p and q of the section to the unit states (1, 0) and (0, 1) over one block of 64 samples,
    the block's state matrix M as P_0, its squarings P_1 .. P_5, and Q_i = M Q_{i-1} for i = 0 .. 64.
    sos: [S, 6] in scipy's layout with a0 == 1."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] < 1:
        raise ValueError("fs2amd: sos must be a float64 [S >= 1, 6] array")
    if not np.all(sos[:, 3] == 1.0) or not np.all(np.isfinite(sos)):
        raise ValueError("fs2amd: every section needs a0 == 1 and finite coefficients")

    def mm(A, B):  # row-major 2x2: two products, one add
        return [A[0] * B[0] + A[1] * B[2], A[0] * B[1] + A[1] * B[3], A[2] * B[0] + A[3] * B[2], A[2] * B[1] + A[3] * B[3]]

    out = np.empty((sos.shape[0], SOS_TABLE_LEN), dtype=np.float64)
    for s, sec in enumerate(sos.tolist()):
        a1, a2 = sec[4], sec[5]
        resp, end = [], []
        for z1, z2 in ((1.0, 0.0), (0.0, 1.0)):
            ys = []
            for _ in range(SOS_BLOCK):
                y = z1
                z1 = z2 - a1 * y
                z2 = -(a2 * y)
                ys.append(y)
            resp.append(ys)
            end.append((z1, z2))
        M = [end[0][0], end[1][0], end[0][1], end[1][1]]
        pows = [M]
        for _ in range(5):
            pows.append(mm(pows[-1], pows[-1]))
        Qi = [[1.0, 0.0, 0.0, 1.0]]
        for _ in range(SOS_BLOCK):
            Qi.append(mm(M, Qi[-1]))
        out[s] = np.array(resp[0] + resp[1] + [v for P in pows for v in P] + [v for Q in Qi for v in Q])
    return out
