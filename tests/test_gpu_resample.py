"""Resampling and peak normalisation on the GPU (include/fs2hip_resample.h, ops.resample,
ops.peak_int16, fs2amd.prepare_wavs, the new keys of build_corpus) against the numpy restatement of
tests/_resample.py and scipy's outputs stored in tests/golden/resample_a.npz.

The order of every sum is fixed by the header, so everything is compared bit for bit: y with
scipy's float64 output, y32 / peak / int16 rows with the restatement's."""
import filecmp
import os

import numpy as np
import pytest
import torch

import _resample as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def taps_dev(up, down):
    from fs2amd.audio import resample_taps

    return None if up == down == 1 else dev(resample_taps(up, down) * up)


def launch(wav, lens, up, down, max_wav_value=R.MAX_WAV_VALUE, want_y=True):
    """(y, y32, peak, out_lens, q) on the host of one launch pair."""
    from fs2amd import ops

    wav = wav if torch.is_tensor(wav) else dev(wav)
    lens = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int64))
    o = ops.resample(wav, lens, up=up, down=down, taps=taps_dev(up, down), want_y=want_y)
    q = ops.peak_int16(o.y32, o.peak, o.out_lens, max_wav_value=max_wav_value)
    return (None if o.y is None else o.y.cpu().numpy(), o.y32.cpu().numpy(), o.peak.cpu().numpy(),
            o.out_lens.cpu().numpy(), q.cpu().numpy())


def check_rows(got, wavs, up, down, refs=None, max_wav_value=R.MAX_WAV_VALUE):
    """Every row of a launch against the restatement (and scipy's stored output where given)."""
    y, y32, peak, out_lens, q = got
    h = R.taps(up, down) * up
    M_max = R.out_len(max(max(len(w) for w in wavs), 1), up, down)
    assert y32.shape == q.shape == (len(wavs), M_max) and peak.shape == out_lens.shape == (len(wavs),)
    assert (y32.dtype, peak.dtype, out_lens.dtype, q.dtype) == (np.float32, np.float32, np.int64, np.int16)
    for b, w in enumerate(wavs):
        ry, ry32, rpeak, rq = R.prepare(w, up, down, h, max_wav_value)
        M = len(ry)
        assert out_lens[b] == M == R.out_len(len(w), up, down)
        if refs is not None:
            same_bits(ry, refs[b])
        if y is not None:
            same_bits(y[b, :M], ry)
            assert (bits(y[b, M:]) == 0).all()
        same_bits(y32[b, :M], ry32)
        same_bits(peak[b], rpeak)
        same_bits(q[b, :M], rq)
        assert (bits(y32[b, M:]) == 0).all() and (q[b, M:] == 0).all()
        assert np.isfinite(y32[b]).all() and np.isfinite(peak[b])


@pytest.fixture(scope="module")
def run_main(fx):
    """Every int16 case of 441/320 in one launch."""
    return launch(fx["wav_441_320"], fx["lens_441_320"], 441, 320)


@pytest.mark.parametrize("up,down", R.RATIOS)
def test_int16_cases_are_scipys_bits(fx, up, down):
    names, wavs, ys = R.cases_of(fx, up, down)
    k = R.key(up, down)
    got = launch(fx["wav_" + k], fx["lens_" + k], up, down)
    same_bits(got[0], fx["y_" + k])  # the whole padded block: scipy's rows, zeros past M_b
    check_rows(got, wavs, up, down, refs=ys)
    silent = [b for b, w in enumerate(wavs) if not w.any()]  # the silent and the empty utterance
    assert len(silent) >= 2
    for b in silent:
        assert got[2][b] == 0 and not got[1][b].any() and not got[4][b].any()
    assert (np.abs(got[4].astype(np.int32)).max(axis=1)[[b for b in range(len(wavs)) if b not in silent]] >= 32767).all()


def test_float32_twin_is_the_int16_case_scaled(fx, run_main):
    got = launch(fx["wav32"], fx["lens32"], 441, 320)
    t, M = int(fx["twin"]), R.out_len(int(fx["lens32"][0]), 441, 320)
    same_bits(got[0][0, :M] * 32768.0, run_main[0][t, :M])
    same_bits(got[0][0, :M], run_main[0][t, :M] * 2.0 ** -15)
    same_bits(got[4][0, :M], run_main[4][t, :M])
    # the general float32 case: the restatement's bits, which are scipy's
    check_rows(got, [fx["wav32"][b, :n] for b, n in enumerate(fx["lens32"])], 441, 320)
    Mg = len(fx["y_general"])
    same_bits(got[0][1, :Mg], fx["y_general"])
    # float32 at 320/441: a tile's input span does not fit behind the taps in LDS, so the samples
    # come from global memory; the bits are the same
    wav16 = fx["wav_320_441"]
    got = launch((wav16.astype(np.float64) / 32768.0).astype(np.float32), fx["lens_320_441"], 320, 441)
    same_bits(got[0] * 32768.0, fx["y_320_441"])
    same_bits(got[4], launch(wav16, fx["lens_320_441"], 320, 441)[4])


def test_an_utterance_does_not_depend_on_its_batch(fx, run_main):
    from fs2amd import ops

    names, wavs, _ = R.cases_of(fx, 441, 320)
    for name in ("tone_noise", "noise_321"):
        b = names.index(name)
        w = wavs[b]
        M = R.out_len(len(w), 441, 320)
        alone = launch(w[None, :], None, 441, 320)  # lens None: the full row
        first = launch(np.stack([fx["wav_441_320"][b], fx["wav_441_320"][1], fx["wav_441_320"][5]]),
                       [len(w), len(wavs[1]), len(wavs[5])], 441, 320)
        # last in a wider batch: a larger n_max and a row stride beyond it, rubbish past the length
        buf = torch.full((4, 12000), 12345, dtype=torch.int16, device=DEV)
        view = buf[:, :11000]
        view[:3, :fx["wav_441_320"].shape[1]] = dev(fx["wav_441_320"][:3])
        view[3, :len(w)] = dev(w)
        lens = [len(wavs[0]), len(wavs[1]), len(wavs[2]), len(w)]
        last = launch(view, lens, 441, 320)
        nulls = launch(view, lens, 441, 320, want_y=False)  # the f64 output NULL
        assert nulls[0] is None
        for k in (0, 1, 4):
            same_bits(alone[k][0][:M], run_main[k][b, :M])
            same_bits(first[k][0][:M], run_main[k][b, :M])
            same_bits(last[k][3][:M], run_main[k][b, :M])
            assert not last[k][3][M:].any()
            if k:
                same_bits(nulls[k], last[k])
        for r in (alone, first):
            same_bits(r[2][0], run_main[2][b])
        same_bits(last[2][3], run_main[2][b])
        same_bits(nulls[2], last[2])
        assert alone[3][0] == first[3][0] == last[3][3] == M


def test_nothing_outside_the_extents_is_written_and_nothing_inside_left(fx, run_main):
    from fs2amd import ops

    wav, lens = fx["wav_441_320"], fx["lens_441_320"]
    B, M_max = wav.shape[0], R.out_len(wav.shape[1], 441, 320)
    nan = float("nan")
    ybuf = torch.full((GUARD + B * M_max + GUARD,), nan, dtype=torch.float64, device=DEV)
    fbuf = torch.full((GUARD + B * M_max + GUARD,), nan, dtype=torch.float32, device=DEV)
    pbuf = torch.full((GUARD + B + GUARD,), nan, dtype=torch.float32, device=DEV)
    lbuf = torch.full((GUARD + B + GUARD,), -7, dtype=torch.int64, device=DEV)
    qbuf = torch.full((GUARD + B * M_max + GUARD,), -7, dtype=torch.int16, device=DEV)
    y, y32 = (t[GUARD:GUARD + B * M_max].view(B, M_max) for t in (ybuf, fbuf))
    peak, out_lens = pbuf[GUARD:GUARD + B], lbuf[GUARD:GUARD + B]
    q = qbuf[GUARD:GUARD + B * M_max].view(B, M_max)
    ops.resample(dev(wav), torch.from_numpy(lens), up=441, down=320, taps=taps_dev(441, 320), out=(y, y32, peak, out_lens))
    ops.peak_int16(y32, peak, out_lens, out=q)
    for buf, inner in ((ybuf, y), (fbuf, y32), (pbuf, peak)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all() and not torch.isnan(inner).any()
    for buf in (lbuf, qbuf):
        assert (buf[:GUARD] == -7).all() and (buf[-GUARD:] == -7).all()
    for k, t in enumerate((y, y32, peak, out_lens, q)):
        same_bits(t.cpu().numpy(), run_main[k])


def test_long_utterance_is_indexed_in_64_bits(fx):
    from fs2amd import ops

    up, down, n, k0, margin = 441, 320, 5200000, 15500, 320
    rng = np.random.default_rng(17)
    burst = rng.integers(-20000, 20000, 2000).astype(np.int16)
    half = R.half_len(up, down)
    assert margin > half // up + 1 and (k0 * up) * down > 2 ** 31  # m * down passes 2^31 inside the window
    short = np.concatenate([np.zeros(margin, np.int16), burst, np.zeros(margin, np.int16)])
    ref = R.resample(short, up, down, R.taps(up, down) * up)
    wav = torch.zeros(1, n, dtype=torch.int16, device=DEV)
    wav[0, k0 * down:k0 * down + len(burst)] = dev(burst)
    o = ops.resample(wav, None, up=up, down=down, taps=taps_dev(up, down))
    M = R.out_len(n, up, down)
    assert o.y.shape == (1, M) and int(o.out_lens[0]) == M and M * down > 2 ** 31
    w0 = (k0 * down - margin) * up // down  # the short case's first output: (k0 - 1) * 441
    assert w0 == (k0 - 1) * up
    window = o.y[0, w0:w0 + len(ref)].cpu().numpy()
    same_bits(window, ref)  # includes the outputs from k0 * 441 on, the burst's own
    assert np.abs(window).max() > 1000
    ybits, fbits = o.y[0].view(torch.int64), o.y32[0].view(torch.int32)
    assert int((ybits[:w0] != 0).sum()) == 0 and int((ybits[w0 + len(ref):] != 0).sum()) == 0
    assert int((fbits[:w0] != 0).sum()) == 0 and int((fbits[w0 + len(ref):] != 0).sum()) == 0
    ry32, rpeak = R.peak_of(ref)
    same_bits(o.peak.cpu().numpy()[0], rpeak)
    q = ops.peak_int16(o.y32, o.peak, o.out_lens)
    same_bits(q[0, w0:w0 + len(ref)].cpu().numpy(), R.to_int16(ry32, rpeak))
    assert int((q[0, :w0] != 0).sum()) == 0 and int((q[0, w0 + len(ref):] != 0).sum()) == 0


def test_equal_rates_skip_the_fir(fx):
    names, wavs, _ = R.cases_of(fx, 441, 320)
    got = launch(fx["wav_441_320"], fx["lens_441_320"], 1, 1)
    assert got[0].shape == fx["wav_441_320"].shape
    same_bits(got[0], fx["wav_441_320"].astype(np.float64))  # samples unchanged before scaling
    check_rows(got, wavs, 1, 1)
    got32 = launch(fx["wav32"], fx["lens32"], 1, 1, max_wav_value=1000.0)
    same_bits(got32[1], fx["wav32"])
    check_rows(got32, [fx["wav32"][b, :n] for b, n in enumerate(fx["lens32"])], 1, 1, max_wav_value=1000.0)


def test_prepare_wavs_over_a_mixed_rate_list(fx):
    import fs2amd

    rates = {(441, 320): 16000, (147, 320): 48000, (1, 2): 44100, (441, 160): 8000, (147, 160): 24000}
    wavs, srcs, want = [], [], []
    for (up, down), rate in rates.items():
        assert R.ratio(R.TARGET, rate) == (up, down)
        names, ws, _ = R.cases_of(fx, up, down)
        k = R.key(up, down)
        q = launch(fx["wav_" + k], fx["lens_" + k], up, down)[4]  # the single-rate launch
        for b in (names.index("tone_noise"), names.index("silence"), names.index("empty"), names.index("two")):
            wavs.append(ws[b])
            srcs.append(rate)
            want.append(q[b, :R.out_len(len(ws[b]), up, down)])
    same_rate = fx["wav_1_2"][-1]  # already at the target rate: only peak-normalised
    wavs.append(same_rate)
    srcs.append(R.TARGET)
    want.append(R.prepare(same_rate, 1, 1, None)[3])
    wavs.append(fx["wav32"][1, :fx["lens32"][1]])  # a float32 waveform among int16 ones of its rate
    srcs.append(16000)
    want.append(R.prepare(wavs[-1], 441, 320, R.taps(441, 320) * 441)[3])
    order = np.random.default_rng(2).permutation(len(wavs))  # the rates interleaved
    got = fs2amd.prepare_wavs([wavs[i] for i in order], [srcs[i] for i in order], sampling_rate=R.TARGET, device=DEV)
    assert len(got) == len(order)
    for g, i in zip(got, order):
        assert g.dtype == np.int16
        same_bits(g, want[i])
    assert fs2amd.prepare_wavs([], [], sampling_rate=R.TARGET, device=DEV) == []
    one = fs2amd.prepare_wavs(wavs[:2], 16000, sampling_rate=R.TARGET, device=DEV)  # one rate for all
    same_bits(one[0], want[0])
    same_bits(one[1], want[1])


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _same_trees(a, b):
    files = _tree(a)
    assert files == _tree(b) and len(files) > 5
    match, mismatch, errors = filecmp.cmpfiles(a, b, files, shallow=False)
    assert not mismatch and not errors and len(match) == len(files), (mismatch, errors)


def test_build_corpus_takes_raw_audio_and_alignment_cuts(tmp_path):
    import fs2amd
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "a"))
    sr = pc["preprocessing"]["audio"]["sampling_rate"]
    assert sr == R.TARGET
    utts = [{k: v for k, v in u.items() if k != "f0"} for u in _utterances(np.random.default_rng(5))]
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    kw = dict(stft=stft, val_size=2, seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)

    def corpus(tag, us):
        lines = fs2amd.build_corpus(str(tmp_path / tag), us, pc, **kw)
        assert len(lines) >= 4  # an utterance is dropped only where YIN finds at most one voiced frame
        return str(tmp_path / tag)

    # raw 16 kHz (and one 48 kHz) recordings of the right duration: 256 * frames samples at 22050 Hz
    rng = np.random.default_rng(8)
    raw = []
    for i, u in enumerate(utts):
        rate = 48000 if i == 3 else 16000
        n = -(-len(u["wav"]) * rate // sr) + rate // 50  # 20 ms to spare for the cuts below
        t = np.arange(n) / rate
        w = 0.4 * np.sin(2 * np.pi * (150.0 + 20 * i) * t) * (0.3 + 0.7 * np.abs(np.sin(3.0 * t + i))) \
            + 0.02 * rng.standard_normal(n)
        w = np.round(9000 * w).astype(np.int16) if i % 2 else w.astype(np.float32)
        raw.append(dict(u, wav=w, sampling_rate=rate))
    ready = fs2amd.prepare_wavs([u["wav"] for u in raw], [u["sampling_rate"] for u in raw], sampling_rate=sr, device=DEV)
    assert all(w.dtype == np.int16 and len(w) >= 256 * int(u["durations"].sum()) for w, u in zip(ready, raw))
    given = [{k: v for k, v in dict(u, wav=w).items() if k != "sampling_rate"} for u, w in zip(raw, ready)]
    _same_trees(corpus("raw", raw), corpus("prepared", given))

    # start / end: the cut of the alignment, against the caller slicing up front
    lead, tail = 0.0371, 0.0123
    padded, cut = [], []
    for u, w in zip(given, ready):
        n0 = int(sr * lead)
        end = lead + len(w) / sr
        long = np.concatenate([np.full(n0, 77, np.int16), w, np.full(int(sr * tail) + 3, -55, np.int16)])
        padded.append(dict(u, wav=long, start=lead, end=end))
        cut.append(dict(u, wav=long[int(sr * lead):int(sr * end)]))
    _same_trees(corpus("aligned", padded), corpus("sliced", cut))
    # both at once: raw audio with its own rate, cut after it is prepared
    both = [dict(u, start=0.01, end=0.01 + 256 * int(u["durations"].sum()) / sr) for u in raw]
    sliced = [dict(g, wav=g["wav"][int(sr * b["start"]):int(sr * b["end"])]) for g, b in zip(given, both)]
    _same_trees(corpus("both", both), corpus("both_sliced", sliced))

    # none of the new keys: what the function did before them (None counts as absent)
    plain = corpus("plain", utts)
    _same_trees(plain, corpus("nones", [dict(u, sampling_rate=None, start=None, end=None) for u in utts]))
    assert _tree(plain) == _tree(str(tmp_path / "raw"))
