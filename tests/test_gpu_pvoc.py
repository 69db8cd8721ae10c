"""The phase vocoder on the GPU (include/fs2hip_pvoc.h, ops.phase_vocoder, fs2amd.time_stretch /
pitch_shift / augment_utterances) against the numpy restatement of tests/_pvoc.py and its recorded
outputs in tests/golden/pvoc_a.npz.

The order of every operation is fixed by the header, so everything is compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import _pvoc as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float32: -7.25, torch.int64: -(1 << 40) - 3}
NB = 5


@pytest.fixture(scope="module")
def fx():
    return V.load_fixture()


@pytest.fixture(scope="module")
def stft():
    import fs2amd

    return fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


class Guarded:
    """A contiguous tensor of ``shape`` with GUARD sentinel elements before and behind it."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        self.n = n

    def _is_sentinel(self, t):
        return bool((t.cpu() == torch.tensor(SENTINEL[self.buf.dtype], dtype=self.buf.dtype)).all())

    def intact(self):
        return self._is_sentinel(self.buf[:GUARD]) and self._is_sentinel(self.buf[GUARD + self.n:])

    def untouched(self):
        return self.intact() and self._is_sentinel(self.view)


def launch(rows, *, T_max=None, J_max=None, spec_pad=0, out_pad=0, frames="host", rates="host"):
    """One launch over rows of (spec f32 [2 NB, >= T], T, rate) with guarded outputs:
    (recomb [B, 2 NB, J_max], frames_out [B]) on the host. Columns of spec at or past a row's T, which
    the kernel must not read, hold NaN; spec_pad / out_pad: elements between the rows beyond T_max /
    J_max, which the kernel must not write."""
    from fs2amd import ops

    B, nb2 = len(rows), rows[0][0].shape[0]
    T_max = T_max or max(max(T for _, T, _ in rows), 1)
    Js = [V.frames(T, r) for _, T, r in rows]
    J_max = J_max or max(Js + [1])
    spec = np.full((B, nb2, T_max + spec_pad), np.nan, dtype=np.float32)
    for b, (s, T, _) in enumerate(rows):
        spec[b, :, :T] = s[:, :T]
    spec_dev = dev(spec)[:, :, :T_max]
    gR, gF = Guarded((B, nb2, J_max + out_pad), torch.float32), Guarded((B,), torch.int64)
    T_arr = np.array([T for _, T, _ in rows], dtype=np.int64)
    r_arr = np.array([r for _, _, r in rows], dtype=np.float64)
    f_arg = {"host": torch.from_numpy(T_arr), "device": dev(T_arr), "none": None}[frames]
    r_arg = torch.from_numpy(r_arr) if rates == "host" else dev(r_arr)
    recomb, frames_out = ops.phase_vocoder(spec_dev, f_arg, r_arg, J_max=J_max, out=(gR.view[:, :, :J_max], gF.view))
    torch.cuda.synchronize()
    assert gR.intact() and gF.intact()
    assert gR._is_sentinel(gR.view[:, :, J_max:])  # between the rows
    return recomb.cpu().numpy(), frames_out.cpu().numpy()


def check(got, rows, refs=None):
    """Every row against the restatement (and a recorded output where given): values bit for bit, +0.0 in
    the columns behind, the true count."""
    recomb, frames_out = got
    for b, (spec, T, rate) in enumerate(rows):
        ref = V.pvoc(spec, T, rate)
        J = ref.shape[1]
        assert frames_out[b] == J == V.frames(T, rate)
        w = min(J, recomb.shape[2])
        same_bits(recomb[b, :, :w], ref[:, :w])
        assert (bits(recomb[b, :, w:]) == 0).all()
        if refs is not None and refs[b] is not None:
            same_bits(recomb[b, :, :w], refs[b][:, :w])


@pytest.mark.parametrize("T", V.KERNEL_T + (129,))
def test_kernel_sizes(fx, T):
    cases = [c for c in V.kernel_cases(NB) if c[2] == T]
    assert len(cases) == (1 if T == 129 else len(V.KERNEL_RATES))
    rows = [(spec, T, rate) for _, spec, T, rate in cases]
    got = launch(rows)
    check(got, rows, refs=[fx["out_" + name] for name, *_ in cases])
    if T == 130:
        assert got[1].tolist() == [520, 260, 130, 123, 87, 65, 36]  # the carry crosses eight blocks at rate 0.25
    if T in (1, 64):  # at rate 1 the last i + 1 is the pad frame: the last column is the last input frame
        j = [r for _, _, r in rows].index(1.0)
        assert got[1][j] == T
        spec = rows[j][0]
        assert np.abs(got[0][j, :, T - 1] - spec[:, T - 1]).max() <= 2.0 ** -23 * np.abs(spec[:, T - 1]).max()


def test_kernel_counts_cover_the_block_edges(fx):
    counts = {int(fx["J_" + name]) for name, *_ in V.kernel_cases(NB)}
    assert {0, 1, 63, 64, 65, 128, 129, 520} <= counts


@pytest.mark.parametrize("frames,rates", (("host", "host"), ("device", "device")))
def test_ragged_batch(fx, frames, rates):
    rows = V.ragged_rows(NB)
    assert len(rows) == 7 and [T for _, T, _ in rows].count(0) == 1
    got = launch(rows, T_max=141, J_max=601, spec_pad=7, out_pad=5, frames=frames, rates=rates)
    check(got, rows, refs=[fx[f"out_ragged_{b}"] for b in range(7)])
    assert got[1].tolist() == [520, V.frames(64, V.SEMITONE), 0, 0, 0, 28, 2]  # rates 0 and NaN, and no frames: 0
    assert (bits(got[0][2:5]) == 0).all()


def test_frames_none_is_t_max_each():
    spec = V.random_spec(NB, 70, 61)
    rows = [(spec, 70, 0.8), (V.random_spec(NB, 70, 62), 70, 1.9)]
    got = launch(rows, frames="none")
    check(got, rows)


def test_layout_independence():
    rows = V.ragged_rows(NB)
    row = rows[5]  # 100 frames at rate 3.7
    long = rows[0]  # 130 frames at rate 0.25: 520 output frames
    for one in (row, long):
        alone = launch([one])
        J = alone[1][0]
        others = [r for r in rows if r is not one]
        for got, b in ((launch([one] + others), 0), (launch(others + [one]), 6), (launch(others[:3] + [one] + others[3:]), 3),
                       (launch([one], T_max=333, J_max=J + 77, spec_pad=13, out_pad=3), 0),
                       (launch([one, others[1]], T_max=131, J_max=J + 1, frames="device", rates="device"), 0)):
            assert got[1][b] == J
            same_bits(got[0][b, :, :J], alone[0][0])
            assert (bits(got[0][b, :, J:]) == 0).all()
    # more bins than a workgroup's four, and a bin count that is no multiple of four
    wide = V.random_spec(11, 90, 77)
    got = launch([(wide, 90, 0.7), (wide, 45, 1.3)])
    check(got, [(wide, 90, 0.7), (wide, 45, 1.3)])
    sub = np.concatenate([wide[2:3], wide[13:14]], 0)  # bin 2 on its own
    one = launch([(sub, 90, 0.7)])
    same_bits(one[0][0, 0], got[0][0, 2, :one[1][0]])
    same_bits(one[0][0, 1], got[0][0, 13, :one[1][0]])


def test_extreme_values(fx):
    spec = V.extreme_spec(NB, 70)
    assert (spec == 0).any() and np.abs(spec).max() == np.float32(1e30) and (np.abs(spec[spec != 0]).min() < 1e-30)
    rows = [(spec, 70, 0.9), (spec, 70, 1.7), (V.zero_frames_spec(NB, 40), 40, 0.8), (V.zero_frames_spec(NB, 40), 40, 1.25)]
    got = launch(rows)
    check(got, rows, refs=[fx["out_extreme_0.9"], fx["out_extreme_1.7"], fx["out_zero_frames_0.8"],
                           fx["out_zero_frames_1.25"]])
    assert np.isfinite(got[0]).all()
    assert np.abs(got[0][0, 1]).max() > 1e29 and 0 < np.abs(got[0][0, 2]).max() < 1e-29


def test_a_count_beyond_j_max_is_cut_where_the_host_cannot_see_it():
    rows = V.ragged_rows(NB)[:2]  # 520 and 61 output frames
    got = launch(rows, J_max=100, out_pad=4, frames="device", rates="device")
    assert got[0].shape == (2, 2 * NB, 100) and got[1].tolist() == [520, V.frames(64, V.SEMITONE)]
    check(got, rows)
    from fs2amd import ops

    spec = dev(np.stack([r[0][:, :64] for r in rows]))
    with pytest.raises(RuntimeError, match="fs2_phase_vocoder"):  # the same, visible to the host: refused
        ops.phase_vocoder(spec, [64, 64], [0.25, 1.0], J_max=100)


def test_error_returns_leave_the_outputs_untouched():
    """Argument checks only: every call below is refused before anything is launched."""
    import ctypes

    from fs2amd import _lib, ops

    lib = _lib.load()
    E, U = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    B, T_max, J_max = 3, 64, 128
    spec = dev(np.ones((B, 2 * NB, T_max), dtype=np.float32))
    rates = dev(np.full(B, 0.5))
    frames = dev(np.array([10, 100, -3], dtype=np.int64))
    gR, gF = Guarded((B, 2 * NB, J_max), torch.float32), Guarded((B,), torch.int64)
    frames_host = (ctypes.c_int64 * 3)(10, 100, -3)
    rates_host = (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    stream = ops._stream(spec)

    def call(**kw):
        d = _lib.PvocDesc()
        d.spec, d.spec_row_stride, d.rates = spec.data_ptr(), T_max, rates.data_ptr()
        d.recomb, d.recomb_row_stride, d.frames_out = gR.view.data_ptr(), J_max, gF.view.data_ptr()
        d.B, d.NB, d.T_max, d.J_max = B, NB, T_max, J_max
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fs2_phase_vocoder(ctypes.byref(d), stream)

    assert lib.fs2_phase_vocoder(None, stream) == E
    seen = dict(frames=frames.data_ptr(), frames_host=ctypes.addressof(frames_host), rates_host=ctypes.addressof(rates_host))
    for kw in (dict(spec=None), dict(rates=None), dict(recomb=None), dict(B=0), dict(B=-2), dict(NB=0), dict(NB=-1),
               dict(T_max=0), dict(J_max=0), dict(J_max=-5), dict(spec_row_stride=T_max - 1),
               dict(recomb_row_stride=J_max - 1), dict(seen, J_max=127, recomb_row_stride=127),
               dict(seen, J_max=20), dict(rates_host=ctypes.addressof(rates_host), J_max=127)):
        assert call(**kw) == E, kw
    assert call(B=65536) == U
    torch.cuda.synchronize()
    assert gR.untouched() and gF.untouched()
    # the wrapper refuses the same things with exceptions
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec[:, :2 * NB - 1], None, rates)
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec, None, rates[:2])
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec, None, rates, J_max=0)
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec.transpose(1, 2).contiguous().transpose(1, 2), None, rates)
    with pytest.raises(RuntimeError, match="fs2_phase_vocoder"):
        ops.phase_vocoder(spec, None, [0.5, 0.5, 0.5], J_max=127)
    assert gR.untouched() and gF.untouched()
    # and the same descriptor, valid, runs: 20, 128 and 0 output frames
    assert call(**seen) == _lib.FS2_OK
    torch.cuda.synchronize()
    assert gF.view.cpu().tolist() == [20, 128, 0] and gR.intact()


WAVE_LENGTHS = (300, 5000, 17920)


def reference_stretch(wavs, rates, stft):
    """ops.stft -> the restatement -> ops.istft -> cut / pad, per waveform of a list of float32 arrays."""
    from fs2amd import ops

    n_max = max(len(w) for w in wavs)
    wav = np.zeros((len(wavs), n_max), dtype=np.float32)
    for b, w in enumerate(wavs):
        wav[b, :len(w)] = w
    lens = torch.tensor([len(w) for w in wavs], dtype=torch.int64)
    o = ops.stft(dev(wav), lens, stft=stft, want=("spec",))
    spec, T = o.spec.cpu().numpy(), o.frames.cpu().numpy()
    outs = [V.pvoc(spec[b], int(T[b]), r) for b, r in enumerate(rates)]
    J = [x.shape[1] for x in outs]
    recomb = np.zeros((len(wavs), spec.shape[1], max(J + [1])), dtype=np.float32)
    for b, x in enumerate(outs):
        recomb[b, :, :J[b]] = x
    y, y_lens = ops.istft(dev(recomb), torch.tensor(J, dtype=torch.int64), stft=stft)
    y, y_lens = y.cpu().numpy(), y_lens.cpu().numpy()
    return [V.cut_pad(y[b, :int(y_lens[b])], V.stretch_len(len(w), r)) for b, (w, r) in enumerate(zip(wavs, rates))], T


def test_time_stretch(stft):
    import fs2amd

    wavs = [V.waveform(n, 3 + i) for i, n in enumerate(WAVE_LENGTHS)]
    for rates in ([0.8] * 3, [1.0] * 3, [1.25] * 3, [1.25, 0.8, 1.0]):
        want, T = reference_stretch(wavs, rates, stft)
        assert T.tolist() == [0, 20, 71]  # 300 samples are too few for a frame
        arg = rates[0] if len(set(rates)) == 1 else rates
        got = fs2amd.time_stretch(wavs, arg, stft=stft, device=DEV)
        for g, w, x, r in zip(got, want, wavs, rates):
            assert g.dtype == np.float32 and len(g) == int(round(len(x) / r))
            same_bits(g, w)
        assert not got[0].any() and np.abs(got[2]).max() > 0.1
    # at rate 1 the waveform comes back, but for the frames the inverse transform cannot rebuild at its ends
    same = fs2amd.time_stretch(wavs[2:], 1.0, stft=stft, device=DEV)[0]
    assert np.abs(same[1024:-1024] - wavs[2][1024:-1024]).max() < 1e-3
    # int16 is widened by / 32768; the order of the list does not matter
    i16 = V.waveform(5000, 4, np.int16)
    a = fs2amd.time_stretch([i16, wavs[2]], [0.8, 1.25], stft=stft, device=DEV)
    b = fs2amd.time_stretch([wavs[2], i16.astype(np.float32) / np.float32(32768.0)], [1.25, 0.8], stft=stft, device=DEV)
    same_bits(a[0], b[1])
    same_bits(a[1], b[0])
    assert a[0].dtype == np.float32 and len(a[0]) == 6250
    assert fs2amd.time_stretch([], 0.9, stft=stft, device=DEV) == []
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fs2amd.time_stretch(wavs, bad, stft=stft, device=DEV)
    with pytest.raises(ValueError):
        fs2amd.time_stretch(wavs, [0.9, 0.8], stft=stft, device=DEV)


def peak_hz(x, sr=22050.0):
    spec = np.abs(np.fft.rfft(x.astype(np.float64) * np.hanning(len(x))))
    return float(np.argmax(spec)) * sr / len(x)


def test_sine_keeps_its_pitch_when_stretched_and_moves_when_shifted(stft):
    import fs2amd

    sr, n = 22050.0, 22050
    sine = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)).astype(np.float32)
    one_bin = sr / 1024.0
    assert abs(peak_hz(sine) - 440.0) <= 1.0
    slow, fast = fs2amd.time_stretch([sine, sine], [0.5, 2.0], stft=stft, device=DEV)
    assert len(slow) == 2 * n and len(fast) == n // 2
    # the level is not asserted: the running phase starts from frame 0, which the STFT's reflect padding
    # fills with an even extension of this sine, and at a rate below 1 the bins around the peak keep that
    # frame's relative phases and partly cancel (DESIGN 9.9 has the figures)
    for y in (slow, fast):
        assert abs(peak_hz(y) - 440.0) <= one_bin, peak_hz(y)
        assert np.isfinite(y).all() and y.any()
    up, down, kept = fs2amd.pitch_shift([sine, sine, sine], [12, -12, 0], stft=stft, device=DEV)
    assert len(up) == len(down) == len(kept) == n and up.dtype == down.dtype == np.float32
    assert abs(peak_hz(up) - 880.0) <= one_bin, peak_hz(up)
    assert abs(peak_hz(down) - 220.0) <= one_bin, peak_hz(down)
    assert abs(peak_hz(kept) - 440.0) <= one_bin


def test_pitch_shift_keeps_the_length(stft):
    import fs2amd
    from fs2amd import ops
    from fs2amd.audio import resample_taps

    wavs = [V.waveform(n, 8 + i) for i, n in enumerate(WAVE_LENGTHS)] + [V.waveform(5000, 4, np.int16)]
    got = fs2amd.pitch_shift(wavs, 12, stft=stft, device=DEV)
    assert [len(g) for g in got] == [len(w) for w in wavs] and all(g.dtype == np.float32 for g in got)
    # what it is made of: a stretch by 1 / 2 and ops.resample(up=1, down=2)
    floats = wavs[:3] + [wavs[3].astype(np.float32) / np.float32(32768.0)]
    slow = fs2amd.time_stretch(floats, 0.5, stft=stft, device=DEV)
    taps = dev(resample_taps(1, 2) * 1)
    for g, s, w in zip(got, slow, floats):
        y = ops.resample(dev(s[None]), up=1, down=2, taps=taps, want_y=False).y32.cpu().numpy()[0]
        same_bits(g, V.cut_pad(y, len(w)))
    mixed = fs2amd.pitch_shift(wavs, [12, 2, -3.5, 12], stft=stft, device=DEV)
    assert [len(g) for g in mixed] == [len(w) for w in wavs]
    same_bits(mixed[0], got[0])
    same_bits(mixed[3], got[3])
    assert np.abs(mixed[2]).max() > 0.05 and fs2amd.pitch_shift([], 2, stft=stft, device=DEV) == []


def test_augment_utterances_into_build_corpus(tmp_path, stft):
    import fs2amd
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "a"))
    assert pc["preprocessing"]["stft"]["hop_length"] == 256
    utts = _utterances(np.random.default_rng(5), 4)
    utts[1] = dict(utts[1], durations=None)  # stays None: nothing to rescale
    copies = list(fs2amd.augment_utterances(utts, rates=(0.9, 1.1), n_steps=(2,), stft=stft, batch_size=3))
    assert [u["basename"] for u in copies] == [f"utt{i:04d}{s}" for i in range(4) for s in ("", "_ts0.90", "_ts1.10", "_ps+2")]
    slow = fs2amd.time_stretch([u["wav"] for u in utts], 0.9, stft=stft, device=DEV)
    shifted = fs2amd.pitch_shift([u["wav"] for u in utts], 2, stft=stft, device=DEV)
    for i, u in enumerate(utts):
        same, ts, ts2, ps = copies[4 * i:4 * i + 4]
        assert same is u
        same_bits(ts["wav"], slow[i])  # batches of three and of one: the same result per utterance
        same_bits(ps["wav"], shifted[i])
        n_new = int(round(len(u["wav"]) / 0.9))
        assert len(ts["wav"]) == n_new and len(ps["wav"]) == len(u["wav"]) and ts["wav"].dtype == np.float32
        for c in (ts, ts2, ps):
            assert c["f0"] is None and "f0" in c
            assert all(c[k] is u[k] for k in ("speaker", "phones", "raw_text", "aux"))
        if u["durations"] is None:
            assert ts["durations"] is None and ps["durations"] is None
        else:
            same_bits(ts["durations"], V.rescale_durations(u["durations"], 0.9, n_new, 256))
            same_bits(ts2["durations"], V.rescale_durations(u["durations"], 1.1, len(ts2["wav"]), 256))
            assert ps["durations"] is u["durations"]
    # int16 in, int16 copies; start / end cannot be stretched
    i16 = dict(utts[0], wav=np.round(utts[0]["wav"] * 20000.0).astype(np.int16))
    c16 = list(fs2amd.augment_utterances([i16], rates=(0.9,), n_steps=(-1,), stft=stft))
    assert [c["wav"].dtype for c in c16] == [np.int16] * 3 and c16[2]["basename"] == "utt0000_ps-1"
    assert 4000 < np.abs(c16[1]["wav"].astype(np.int64)).max() <= 32767  # the input peaks near 0.5 * 20000
    with pytest.raises(ValueError, match="start / end"):
        list(fs2amd.augment_utterances([dict(utts[0], start=0.0, end=0.1)], rates=(0.9,), stft=stft))
    with pytest.raises(ValueError, match="share a name"):
        list(fs2amd.augment_utterances(utts, rates=(0.9, 0.901), stft=stft))

    given = [u for u in utts if u["durations"] is not None]
    out = str(tmp_path / "corpus")
    lines = fs2amd.build_corpus(out, fs2amd.augment_utterances(given, rates=(0.9,), n_steps=(2,), stft=stft), pc,
                                stft=stft, val_size=2, seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)
    assert len(lines) == 3 * len(given) == 9
    for u in given:
        spk, name = u["speaker"], u["basename"]
        n_new = int(round(len(u["wav"]) / 0.9))
        want = {"": np.asarray(u["durations"]), "_ts0.90": V.rescale_durations(u["durations"], 0.9, n_new, 256),
                "_ps+2": np.asarray(u["durations"])}
        for suffix, d in want.items():
            for kind in ("mel", "pitch", "energy", "duration"):
                assert os.path.exists(os.path.join(out, kind, f"{spk}-{kind}-{name}{suffix}.npy")), (kind, name, suffix)
            dur = np.load(os.path.join(out, "duration", f"{spk}-duration-{name}{suffix}.npy"))
            mel = np.load(os.path.join(out, "mel", f"{spk}-mel-{name}{suffix}.npy"))
            same_bits(dur, d.astype(np.int64))
            n = n_new if suffix == "_ts0.90" else len(u["wav"])
            assert mel.shape == (int(dur.sum()), 80) and dur.sum() <= 1 + n // 256  # the durations fit the mel
            assert any(m.startswith(f"{name}{suffix}|{spk}|") for m in lines)
        slow_mel = np.load(os.path.join(out, "mel", f"{spk}-mel-{name}_ts0.90.npy"))
        assert abs(slow_mel.shape[0] - np.sum(u["durations"]) / 0.9) <= 1.0
