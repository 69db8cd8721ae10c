"""Recursive filtering and BS.1770 loudness on the GPU (include/fs2hip_iir.h, ops.sosfilt,
ops.loudness_gate, ops.gain_int16, fs2amd.integrated_loudness / normalize_loudness, the lufs options of
prepare_wavs and build_corpus) against the numpy restatement of tests/_loudness.py and its recorded
outputs in tests/golden/loudness_a.npz.

The order of every operation is fixed by the header, so everything is compared bit for bit."""
import filecmp
import math
import os

import numpy as np
import pytest
import torch

import _loudness as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float64: -7.25, torch.int32: -12345, torch.int16: -21846, torch.float32: -7.25}
H0 = 2205
TORCH_OF = {np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


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

    def intact(self):
        s = torch.tensor(SENTINEL[self.buf.dtype], dtype=self.buf.dtype)
        return bool((self.buf[:GUARD].cpu() == s).all() and (self.buf[GUARD + self.n:].cpu() == s).all())

    def untouched(self):
        return self.intact() and bool((self.view.cpu() == torch.tensor(SENTINEL[self.buf.dtype], dtype=self.buf.dtype)).all())


def row_of(n, seed, dtype):
    g = np.random.RandomState(seed)
    if dtype == np.int16:
        return np.clip(np.round(g.standard_normal(n) * 5000.0), -32768, 32767).astype(np.int16)
    if dtype == np.float32:
        return (g.standard_normal(n) * 0.2 * np.float32(1.00037)).astype(np.float32)
    return g.standard_normal(n) * 0.3


def poisoned(rows, dtype, pad=0, extra=0):
    """(device view [B, n_max] with row stride n_max + pad, lens): everything no kernel may read is poison."""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    n_max = max(int(lens.max(initial=0)), 1) + extra
    poison = 12345 if dtype == np.int16 else np.nan
    buf = np.full((len(rows), n_max + pad), poison, dtype=dtype)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    return dev(buf)[:, :n_max], lens


def run_sosfilt(rows, sos, dtype, zi=None, pad=0, extra=0):
    """ops.sosfilt over a ragged batch with guarded outputs, checked against the restatement row by row."""
    from fs2amd import ops

    wav, lens = poisoned(rows, dtype, pad, extra)
    B, n_max = wav.shape
    S = len(sos)
    gy, g32, gz = Guarded((B, n_max), torch.float64), Guarded((B, n_max), torch.float32), Guarded((B, S, 2), torch.float64)
    out = ops.sosfilt(wav, sos, dev(lens), zi=None if zi is None else dev(zi), want_y32=True, want_zf=True,
                      out=(gy.view, g32.view, gz.view))
    torch.cuda.synchronize()
    assert gy.intact() and g32.intact() and gz.intact()
    y, y32, zf = out.y.cpu().numpy(), out.y32.cpu().numpy(), out.zf.cpu().numpy()
    for b, x in enumerate(rows):
        ry, rzf = R.sosfilt(x, sos, None if zi is None else zi[b])
        n = len(x)
        same_bits(y[b, :n], ry)
        same_bits(y32[b, :n], ry.astype(np.float32))
        same_bits(zf[b], rzf)
        assert (bits(y[b, n:]) == 0).all() and (bits(y32[b, n:]) == 0).all()
    return y, zf


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_sosfilt_lengths_sections_and_dtypes(S, dtype):
    """B = 7 twice: every length at which a block, a group of 64 blocks or a chunk of 16384 samples ends, one
    short and one past; the first launch from zero state, the second from given states and with a row
    stride beyond n_max."""
    sos = R.sections_for(S)
    assert sos.shape == (S, 6)
    lengths = R.SOS_LENGTHS + (200,)
    assert {0, 1, 63, 64, 65, 4095, 4096, 4097, 8193, 3 * 4096 + 17} <= set(lengths) and len(lengths) == 14
    rows = [row_of(n, 100 + i, dtype) for i, n in enumerate(lengths)]
    run_sosfilt(rows[0::2], sos, dtype)
    zi = np.random.RandomState(7).standard_normal((7, S, 2)) * (100.0 if dtype == np.int16 else 0.01)
    run_sosfilt(rows[1::2], sos, dtype, zi=zi, pad=37, extra=5)


def test_sosfilt_does_not_depend_on_the_batch():
    sos = R.k_weighting(22050)
    x = row_of(3 * 4096 + 17, 3, np.int16)
    others = [row_of(n, 50 + n, np.int16) for n in (5, 40000, 0, 4096, 777, 16385)]
    alone, zf1 = run_sosfilt([x], sos, np.int16)
    inside, zf7 = run_sosfilt(others[:4] + [x] + others[4:], sos, np.int16, pad=11)
    same_bits(alone[0], inside[4, :len(x)])
    same_bits(zf1[0], zf7[4])
    wide, _ = run_sosfilt([x], sos, np.int16, extra=20000)  # another n_max
    same_bits(alone[0], wide[0, :len(x)])


def test_sosfilt_reproduces_the_fixture_and_scipy(fx):
    from scipy import signal

    x, fs = R.fixture_cases()["speech_i16_16000"]
    y, zf = run_sosfilt([x[:5000]], R.k_weighting(fs), np.int16)
    same_bits(y[0], fx["y_speech_i16_16000"])
    same_bits(zf[0], fx["zf_speech_i16_16000"])
    sc = signal.sosfilt(R.k_weighting(fs), x[:5000].astype(np.float64))
    assert np.abs(y[0] - sc).max() <= 2.0 ** -31 * np.abs(sc).max()


def run_gate(ys, H, gate_abs, rel=0.1, extra=0):
    from fs2amd import ops

    lens = np.array([len(y) for y in ys], dtype=np.int64)
    n_max = max(int(lens.max()), 1) + extra
    buf = np.full((len(ys), n_max), np.nan)
    for b, y in enumerate(ys):
        buf[b, :len(y)] = y
    gz, gc = Guarded((len(ys),), torch.float64), Guarded((len(ys), 3), torch.int32)
    out = ops.loudness_gate(dev(buf), dev(lens), hop=H, abs_gate=gate_abs, rel_factor=rel, out=(gz.view, gc.view))
    torch.cuda.synchronize()
    assert gz.intact() and gc.intact()
    zbar, counts = out.zbar.cpu().numpy(), out.counts.cpu().numpy()
    for b, y in enumerate(ys):
        rz, rc = R.gate(y, H, gate_abs, rel)
        same_bits(zbar[b], np.float64(rz))
        assert tuple(counts[b]) == rc, (b, counts[b], rc)
    return zbar, counts


def test_gate_edge_lengths_both_gates_and_silence():
    T = 4 * H0
    g = np.random.RandomState(12)
    ga = R.abs_gate(np.int16)
    two, _ = R.sosfilt(R.two_level_row(22050), R.k_weighting(22050))
    ys = [g.standard_normal(n) * 700.0 for n in (T - 1, T, T + H0 - 1, T + H0)] + [two, np.zeros(3 * 22050),
                                                                                  g.standard_normal(3 * 22050) * 2.0]
    zbar, counts = run_gate(ys, H0, ga)
    assert counts[:4, 0].tolist() == [0, 1, 1, 2] and zbar[0] == 0.0
    assert counts[4].tolist() == [27, 20, 10]           # the silent second under the absolute gate, the quiet one under the relative
    assert counts[5].tolist() == [27, 0, 0] and counts[6].tolist() == [27, 0, 0] and zbar[5] == 0.0 and zbar[6] == 0.0
    assert not np.signbit(zbar).any()
    # a batch in which no row has a block, and one row alone at another n_max
    run_gate([ys[0], g.standard_normal(5)], H0, ga)
    alone, _ = run_gate([two], H0, ga, extra=999)
    same_bits(alone[0], zbar[4])
    # other hops: a multiple of 8, below 8, and a tree deeper than one level of 256 leaves
    for H in (1600, 5, 4800):
        run_gate([g.standard_normal(n) * 300.0 for n in (4 * H, 31 * H + 3, 9 * H - 1)], H, 100.0, rel=0.5)


def run_gain(rows, zbar, tz, ceiling=None, pad=0):
    from fs2amd import ops

    dtype = rows[0].dtype
    wav, lens = poisoned(rows, dtype, pad, extra=3)
    B, n_max = wav.shape
    tdt = TORCH_OF[np.dtype(dtype)]
    gq, gg, gc, gu = Guarded((B, n_max), tdt), Guarded((B,), torch.float64), Guarded((B,), torch.int32), Guarded((B,), torch.int32)
    gp = Guarded((B,), torch.float64) if ceiling else None
    out = ops.gain_int16(wav, dev(np.asarray(zbar, dtype=np.float64)), dev(lens), target_z=tz, peak_ceiling=ceiling,
                         out=(gq.view, gg.view, gc.view, gu.view, gp.view if gp else None))
    torch.cuda.synchronize()
    assert all(g.intact() for g in (gq, gg, gc, gu) + ((gp,) if gp else ()))
    q = out.q.cpu().numpy()
    res = []
    for b, x in enumerate(rows):
        r = R.gain(x, zbar[b], tz, ceiling or 0.0)
        same_bits(q[b, :len(x)], r["q"])
        assert not q[b, len(x):].any()
        same_bits(out.gain.cpu().numpy()[b], np.float64(r["gain"]))
        assert int(out.clipped[b]) == r["clipped"] and int(out.unmeasured[b]) == r["unmeasured"]
        if gp:
            same_bits(out.peak.cpu().numpy()[b], np.float64(r["peak"]))
        res.append(r)
    return res


def test_gain_saturation_ceiling_ties_and_unmeasured():
    rows = [row_of(n, 70 + n, np.int16) for n in (30000, 1, 4097, 0, 2500)]
    rows[4] = (np.arange(2500) - 1250).astype(np.int16)  # with gain 0.5: every tie, both signs
    zbar = [1.0e6, 2.5e7, 0.0, 3.0, 4.0]
    r = run_gain(rows, zbar, 1.0)
    assert r[4]["gain"] == 0.5 and r[2]["unmeasured"] == 1 and r[2]["gain"] == 1.0
    loud = run_gain(rows, [z * 1e-6 for z in zbar], 1.0e2)  # gains of 2 and more: saturation on both sides
    assert loud[0]["clipped"] > 1000 and loud[0]["q"].max() == 32767 and loud[0]["q"].min() == -32768 and loud[2]["clipped"] == 0
    capped = run_gain(rows, [z * 1e-6 for z in zbar], 1.0e2, ceiling=20000.0, pad=9)
    assert capped[0]["clipped"] == 0 and capped[0]["gain"] < loud[0]["gain"] and capped[0]["gain"] == 20000.0 / capped[0]["peak"]
    assert np.abs(capped[0]["q"].astype(np.int32)).max() == 20000
    low = run_gain(rows, zbar, 1.0, ceiling=32768.0)  # a ceiling never raises the gain
    assert [a["gain"] for a in low] == [a["gain"] for a in r]
    frows = [row_of(n, 80 + n, np.float32) for n in (9000, 0, 300)]
    f = run_gain(frows, [0.01, 1.0, 0.0], 1.0, ceiling=1.5)
    assert f[0]["clipped"] == 0 and np.abs(f[0]["q"]).max() > 1.0  # float output is not saturated


def test_integrated_and_normalize_loudness_end_to_end(fx):
    import fs2amd

    cases = R.fixture_cases()
    for fs in (16000, 22050, 8000):
        names = [n for n in sorted(cases) if cases[n][1] == fs]
        wavs = [cases[n][0] for n in names]
        lufs = fs2amd.integrated_loudness(wavs, sampling_rate=fs, device=DEV)
        out, recs = fs2amd.normalize_loudness(wavs, sampling_rate=fs, target_lufs=-23.0, device=DEV)
        for n, w, l, o, rec in zip(names, wavs, lufs, out, recs):
            r = R.normalize(w, fs, -23.0)
            same_bits(np.float64(r["zbar"]), fx["zbar_" + n])
            assert l == r["lufs"] == rec.lufs and (l == -math.inf) == (r["zbar"] == 0.0)
            assert o.dtype == w.dtype
            same_bits(o, r["q"])
            same_bits(o[:2000], fx["q_" + n])
            same_bits(np.float64(rec.gain), fx["gain_" + n])
            assert rec.clipped == int(fx["clipped_" + n]) and rec.unmeasured == bool(r["unmeasured"])
            if rec.unmeasured:
                same_bits(o, w)
            elif rec.clipped == 0:  # int16 rounding (none for float32) is the slack
                again = fs2amd.integrated_loudness([o], sampling_rate=fs, device=DEV)[0]
                print(f"{n}: {l:.3f} LUFS, gain {rec.gain:.4f}, re-measured {again:.4f}")
                assert abs(again - (-23.0)) <= 0.01
    assert fs2amd.integrated_loudness([], sampling_rate=22050, device=DEV) == []
    # the ceiling reaches the kernel as a fraction of full scale
    w = cases["two_level_8000"][0]
    out, recs = fs2amd.normalize_loudness([w], sampling_rate=8000, target_lufs=-3.0, peak_ceiling=0.5, device=DEV)
    r = R.normalize(w, 8000, -3.0, peak_ceiling=0.5)
    same_bits(out[0], r["q"])
    assert recs[0].clipped == 0 and np.abs(out[0].astype(np.int32)).max() == 16384
    # the calibration tone on the device
    tone = fs2amd.integrated_loudness([R.sine_row(48000)], sampling_rate=48000, device=DEV)[0]
    assert abs(tone - (-3.01)) <= 0.05


def test_prepare_wavs_loudness_on_the_device():
    import fs2amd
    import _resample as RS
    import _vad as V

    rfx = RS.load_fixture()
    names, ws, _ = RS.cases_of(rfx, 441, 320)
    w = ws[names.index("tone_noise")]
    reps = -(-16000 // len(w))  # a second of it, so that there are gating blocks
    padded = np.concatenate([np.zeros(4000, np.int16), np.tile(w, reps), np.zeros(5000, np.int16)])
    other = np.concatenate([np.zeros(900, np.int16), ws[names.index("two")], np.zeros(300, np.int16)])  # too short to measure
    args = ([padded, other], 16000)
    plain = fs2amd.prepare_wavs(*args, sampling_rate=RS.TARGET, device=DEV)
    again = fs2amd.prepare_wavs(*args, sampling_rate=RS.TARGET, device=DEV, lufs=None, lufs_peak_ceiling=None)
    for a, p in zip(again, plain):
        same_bits(a, p)
    # resample, peak, (trim,) then the ops chained by hand = the restatement on the plain output
    got = fs2amd.prepare_wavs(*args, sampling_rate=RS.TARGET, device=DEV, lufs=-23.0)
    for g, p in zip(got, plain):
        same_bits(g, R.normalize(p, RS.TARGET, -23.0)["q"])
    same_bits(got[1], plain[1])
    assert R.normalize(plain[0], RS.TARGET, -23.0)["unmeasured"] == 0 and not np.array_equal(got[0], plain[0])
    got = fs2amd.prepare_wavs(*args, sampling_rate=RS.TARGET, device=DEV, trim_db=40.0, lufs=-20.0, lufs_peak_ceiling=0.25)
    for g, p in zip(got, plain):
        s, e = V.analyse(p, frame_length=2048, hop=512, top_db=40.0)["trim"]
        same_bits(g, R.normalize(p[s:e], RS.TARGET, -20.0, peak_ceiling=0.25)["q"])
    assert 0 < len(got[0]) < len(plain[0]) - 8000 and np.abs(got[0].astype(np.int32)).max() <= 8192


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_build_corpus_without_lufs_writes_the_same_bytes(tmp_path):
    import fs2amd
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "a"))
    sr = pc["preprocessing"]["audio"]["sampling_rate"]
    utts = _utterances(np.random.default_rng(5))
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    kw = dict(stft=stft, val_size=2, seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)
    a, b, c = str(tmp_path / "plain"), str(tmp_path / "none"), str(tmp_path / "lufs")
    lines = fs2amd.build_corpus(a, utts, pc, **kw)
    assert fs2amd.build_corpus(b, utts, pc, lufs=None, **kw) == lines and len(lines) == 6
    assert _tree(a) == _tree(b) and len(_tree(a)) > 5
    match, mismatch, errors = filecmp.cmpfiles(a, b, _tree(a), shallow=False)
    assert not mismatch and not errors and len(match) == len(_tree(a))
    # with a target, the utterances that go through prepare_wavs change level and nothing else does
    raw = [dict(u, sampling_rate=sr) for u in utts]
    d = str(tmp_path / "raw")
    fs2amd.build_corpus(d, raw, pc, **kw)
    assert fs2amd.build_corpus(c, raw, pc, lufs=-30.0, **kw) is not None
    assert _tree(c) == _tree(d)
    assert filecmp.cmpfiles(c, d, [f for f in _tree(c) if f.startswith("energy")], shallow=False)[1]


def test_error_returns_leave_the_outputs_untouched():
    """Argument checks only: every call below is refused before anything is launched."""
    from fs2amd import _lib, ops

    lib = _lib.load()
    E, U = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    B, n_max, S, H = 2, 10000, 2, 2205
    wav = dev(np.ones((B, n_max), dtype=np.int16))
    sos, tab = dev(R.k_weighting(22050)), dev(R.tables(R.k_weighting(22050)))
    yin, zin = dev(np.ones((B, n_max))), dev(np.ones(B))
    gy, g32, gzf = Guarded((B, n_max), torch.float64), Guarded((B, n_max), torch.float32), Guarded((B, S, 2), torch.float64)
    gz, gc, gw = Guarded((B,), torch.float64), Guarded((B, 3), torch.int32), Guarded((B * 6,), torch.float64)
    gq, gg, gcl = Guarded((B, n_max), torch.int16), Guarded((B,), torch.float64), Guarded((B,), torch.int32)
    gu, gp = Guarded((B,), torch.int32), Guarded((B,), torch.float64)
    stream, ptr = ops._stream(wav), ops._ptr
    need = _lib.loudness_workspace_bytes(B, n_max, H)
    assert need == 8 * B * 6  # J_max = 1: four sub-block sums and the two tree buffers

    def filt(wav_p=ptr(wav), dtype=_lib.FS2_I16, stride=n_max, B=B, n_max=n_max, sos_p=ptr(sos), tab_p=ptr(tab), S=S,
             y=ptr(gy.view)):
        return lib.fs2_sosfilt(wav_p, dtype, stride, None, B, n_max, sos_p, tab_p, S, None, y, ptr(g32.view), ptr(gzf.view),
                               stream)

    for kw in (dict(wav_p=None), dict(sos_p=None), dict(tab_p=None), dict(y=None), dict(B=0), dict(B=-1), dict(n_max=0),
               dict(S=0), dict(stride=n_max - 1)):
        assert filt(**kw) == E, kw
    for kw in (dict(dtype=_lib.FS2_BF16), dict(dtype=_lib.FS2_FP8), dict(S=9), dict(B=65536)):
        assert filt(**kw) == U, kw

    def gate(y=ptr(yin), B=B, n_max=n_max, H=H, ga=1.0, rel=0.1, zbar=ptr(gz.view), counts=ptr(gc.view), ws=ptr(gw.view),
             ws_bytes=need):
        return lib.fs2_loudness_gate(y, None, B, n_max, H, ga, rel, zbar, counts, ws, ws_bytes, stream)

    for kw in (dict(y=None), dict(zbar=None), dict(counts=None), dict(B=0), dict(n_max=0), dict(H=0), dict(H=-5), dict(ws=None),
               dict(ws_bytes=need - 1), dict(ga=-1.0), dict(ga=float("nan")), dict(rel=-0.1), dict(rel=float("nan"))):
        assert gate(**kw) == E, kw
    for kw in (dict(H=32769), dict(B=65536)):
        assert gate(**kw) == U, kw

    def gain(wav_p=ptr(wav), dtype=_lib.FS2_I16, stride=n_max, B=B, n_max=n_max, zbar=ptr(zin), tz=1.0, ceil=0.0, q=ptr(gq.view),
             g=ptr(gg.view), cl=ptr(gcl.view), peak=ptr(gp.view)):
        return lib.fs2_gain_int16(wav_p, dtype, stride, None, B, n_max, zbar, tz, ceil, q, g, cl, ptr(gu.view), peak, stream)

    for kw in (dict(wav_p=None), dict(zbar=None), dict(q=None), dict(g=None), dict(cl=None), dict(B=0), dict(n_max=0),
               dict(stride=n_max - 1), dict(tz=0.0), dict(tz=-1.0), dict(tz=float("nan")), dict(tz=float("inf")), dict(ceil=-1.0),
               dict(ceil=float("nan")), dict(ceil=100.0, peak=None)):
        assert gain(**kw) == E, kw
    for kw in (dict(dtype=_lib.FS2_F64), dict(dtype=_lib.FS2_BF16), dict(B=65536)):
        assert gain(**kw) == U, kw
    torch.cuda.synchronize()
    for g in (gy, g32, gzf, gz, gc, gw, gq, gg, gcl, gu, gp):
        assert g.untouched()
    # the wrappers refuse the same things with exceptions
    with pytest.raises(ValueError):
        ops.sosfilt(wav, np.ones((9, 6)))
    with pytest.raises(ValueError):
        ops.sosfilt(wav, np.array([[1.0, 0.0, 0.0, 2.0, 0.0, 0.0]]))
    with pytest.raises(ValueError):
        ops.loudness_gate(yin, hop=0, abs_gate=1.0)
    with pytest.raises(ValueError):
        ops.loudness_gate(yin, hop=40000, abs_gate=1.0)
    with pytest.raises(ValueError):
        ops.gain_int16(wav, zin, target_z=0.0)
