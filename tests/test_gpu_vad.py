"""Silence trimming and splitting on the GPU (include/fs2hip_vad.h, ops.frame_power,
ops.activity_intervals, ops.cut_rows, fs2amd.trim_silence / split_silence, the trim options of
prepare_wavs and build_corpus) against the numpy restatement of tests/_vad.py and its recorded outputs
in tests/golden/vad_a.npz.

The order of every sum is fixed by the header, so everything is compared bit for bit."""
import filecmp
import os

import numpy as np
import pytest
import torch

import _vad as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float64: -7.25, torch.uint8: 0xA5, torch.int32: -12345, torch.int64: -(1 << 40) - 3,
            torch.int16: -21846, torch.float32: -7.25}


@pytest.fixture(scope="module")
def fx():
    return V.load_fixture()


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


def launch(rows, *, frame_length=V.L0, hop=V.HOP0, threshold=None, top_db=60.0, floor=None, min_silence=1, margin=0,
           max_intervals=None, chunk_frames=0, n_max=None, dtype=None):
    """The three launches over a ragged batch with guarded outputs, on the host:
    dict(P, Pmax, n_frames, active, count, intervals, trim, rows, out_lens)."""
    from fs2amd import ops

    dtype = dtype or rows[0].dtype
    wav, lens = V.pack(rows, dtype)
    if n_max is not None:
        wav = np.concatenate([wav, np.full((len(rows), n_max - wav.shape[1]), 99, dtype=dtype)], axis=1)  # never read
    B, n_max = wav.shape
    F_max = V.frames(n_max, hop)
    thr = V.threshold_of(top_db) if threshold is None else threshold
    flo = V.floor_of(dtype) if floor is None else floor
    cap = (F_max + 1) // 2 if max_intervals is None else max_intervals
    wav_dev, lens_dev = dev(wav), dev(lens)
    gP, gM = Guarded((B, F_max), torch.float64), Guarded((B,), torch.float64)
    P, Pmax, n_frames = ops.frame_power(wav_dev, lens_dev, frame_length=frame_length, hop_length=hop, out=(gP.view, gM.view))
    gA, gC = Guarded((B, F_max), torch.uint8), Guarded((B,), torch.int32)
    gI, gT = Guarded((B, cap, 2), torch.int64), Guarded((B, 2), torch.int64)
    active, count, intervals, trim = ops.activity_intervals(
        P, Pmax, lens_dev, threshold=thr, floor=flo, hop_length=hop, min_silence=min_silence, margin=margin,
        max_intervals=max_intervals, n_max=n_max, chunk_frames=chunk_frames, out=(gA.view, gC.view, gI.view, gT.view))
    trim_h = trim.cpu().numpy()
    M_max = max(int((trim_h[:, 1] - trim_h[:, 0]).max()), 1)
    tdt = torch.int16 if dtype == np.int16 else torch.float32
    gR = Guarded((B, M_max), tdt)
    cut, out_lens = ops.cut_rows(wav_dev, trim[:, 0].contiguous(), trim[:, 1].contiguous(), out=gR.view)
    torch.cuda.synchronize()
    for g in (gP, gM, gA, gC, gI, gT, gR):
        assert g.intact()
    return dict(P=P.cpu().numpy(), Pmax=Pmax.cpu().numpy(), n_frames=n_frames.cpu().numpy(), active=active.cpu().numpy(),
                count=count.cpu().numpy(), intervals=intervals.cpu().numpy(), trim=trim_h, rows=cut.cpu().numpy(),
                out_lens=out_lens.cpu().numpy(), threshold=thr, floor=flo)


def check(got, rows, refs=None, **kw):
    """Every row of a launch against the restatement (and a recorded result where given): values bit for
    bit, and zeros in the padding of every output."""
    kw = {k: v for k, v in kw.items() if k in ("frame_length", "hop", "min_silence", "margin")}
    cap = got["intervals"].shape[1]
    for b, x in enumerate(rows):
        r = V.analyse(x, threshold=got["threshold"], floor=got["floor"], **kw)
        F = len(r["P"])
        assert got["n_frames"][b] == F
        same_bits(got["P"][b, :F], r["P"])
        assert (bits(got["P"][b, F:]) == 0).all()
        same_bits(got["Pmax"][b], np.float64(r["P"].max(initial=0.0)))
        same_bits(got["active"][b, :F], r["active"].astype(np.uint8))
        assert not got["active"][b, F:].any()
        k = len(r["intervals"])
        assert got["count"][b] == k
        same_bits(got["intervals"][b, :min(k, cap)], r["intervals"][:cap])
        assert not got["intervals"][b, min(k, cap):].any()
        same_bits(got["trim"][b], r["trim"])
        n = int(r["trim"][1] - r["trim"][0])
        assert got["out_lens"][b] == n
        same_bits(got["rows"][b, :n], r["cut"])
        assert not got["rows"][b, n:].any()
        if refs is not None and refs[b] is not None:
            same_bits(got["P"][b, :F], refs[b]["P"])
            same_bits(got["active"][b, :F], refs[b]["act"])
            same_bits(got["intervals"][b, :k], refs[b]["iv"])
            same_bits(got["trim"][b], refs[b]["trim"])


def recorded(fx, name):
    return {k: fx[f"{k}_{name}"] for k in ("P", "act", "iv", "trim")}


def test_row_lengths_in_one_ragged_launch(fx):
    rows = V.length_rows()
    assert [len(x) for x in rows] == list(V.LENGTHS) and len(rows[5]) == 0
    got = launch(rows)
    assert got["P"].shape == (11, V.frames(9001, 256))
    check(got, rows, refs=[recorded(fx, f"len_{b}_{len(x)}") for b, x in enumerate(rows)])
    assert got["trim"][5].tolist() == [0, 0] and got["count"][5] == 0 and got["Pmax"][5] == 0.0


def test_chunk_boundaries_and_chunk_size(fx):
    from fs2amd import _lib

    row = V.chunk_row()
    F = V.frames(len(row), V.HOP0)
    C = _lib.VAD_CHUNK_FRAMES
    assert F > 3 * C and F > 4 * _lib.VAD_TILE_FRAMES  # more than three steps of the walk, more than four power tiles
    ref = recorded(fx, "chunks")
    assert ref["act"][C - 2:C + 2].all() and ref["act"][2 * C - 2:2 * C + 2].all()  # the run and the filled silence
    results = []
    for chunk in (0, 64, 128, 256):
        got = launch([row, row[:70000]], min_silence=3, chunk_frames=chunk)
        check(got, [row, row[:70000]], refs=[ref, None], min_silence=3)
        results.append(got)
    for got in results[1:]:
        for k in ("active", "count", "intervals", "trim"):
            same_bits(got[k], results[0][k])
    raw = launch([row], min_silence=1)  # unfilled: the silence of two frames lies across the second boundary
    assert not raw["active"][0, 2 * C - 1] and not raw["active"][0, 2 * C] and raw["count"][0] == results[0]["count"][0] + 1


def test_content_cases(fx):
    rows = V.content_rows()
    names = [n for n in rows if rows[n].dtype == np.int16]
    got = launch([rows[n] for n in names])
    check(got, [rows[n] for n in names], refs=[recorded(fx, "content_" + n) for n in names])
    i = names.index
    assert got["Pmax"][i("silent")] == 0.0 and got["active"][i("silent")].all()  # ref = floor: nothing is below it
    assert got["active"][i("constant")].all() and got["trim"][i("constant")].tolist() == [0, 4000]
    assert got["active"][i("first_frame")].tolist() == [1, 1, 1] + [0] * 13
    assert got["active"][i("last_frame")].tolist() == [0] * 14 + [1, 1]
    assert got["trim"][i("impulse_0")].tolist() == [0, 768] and got["trim"][i("impulse_last")].tolist() == [3584, 4000]
    below = rows["below_floor"]
    got = launch([below, V.speechlike(3000, 9, np.float32)])
    check(got, [below, V.speechlike(3000, 9, np.float32)], refs=[recorded(fx, "content_below_floor"), None])
    assert 0 < got["Pmax"][0] < got["floor"] and got["active"][0, :16].all()
    # with threshold 1 nothing exceeds the reference: no active frame, (0, 0), an empty cut
    got = launch([rows["silent"], rows["constant"]], threshold=1.0)
    check(got, [rows["silent"], rows["constant"]])
    assert got["trim"].tolist() == [[0, 0], [0, 0]] and got["count"].tolist() == [0, 0] and got["rows"].shape == (2, 1)


def test_dtypes(fx):
    x = V.speechlike(9001, 41)
    twin = (x.astype(np.float64) / 32768.0).astype(np.float32)
    general = V.speechlike(9001, 24, np.float32)
    g = general.astype(np.float64) * 32768.0
    assert (twin.astype(np.float64) * 32768.0 == x).all() and (g != np.round(g)).mean() > 0.9
    a = launch([x, V.speechlike(500, 3)])
    check(a, [x, V.speechlike(500, 3)])
    b = launch([twin, general], top_db=60.0)
    check(b, [twin, general])
    same_bits(a["P"][0], b["P"][0] * 32768.0 ** 2)
    same_bits(a["active"][0], b["active"][0])
    same_bits(a["intervals"][0], b["intervals"][0])
    c = launch([general], top_db=40.0, min_silence=2)
    check(c, [general], refs=[recorded(fx, "top_db_40_f32")], min_silence=2)


@pytest.mark.parametrize("L,hop", V.GEOMETRIES[1:])
def test_geometries(fx, L, hop):
    n = 7013 if hop > 1 else 301
    long = V.chunk_row() if hop > 1 else V.speechlike(700, 33)  # more than one tile of frames and staging pass
    for tag, dt in (("i16", np.int16), ("f32", np.float32)):
        x = V.speechlike(n, 21 if dt == np.int16 else 22, dt)
        rows = [x, long if dt == np.int16 else (long / np.float32(32768.0 * 0.99)).astype(np.float32), x[:n // 3]]
        got = launch(rows, frame_length=L, hop=hop)
        check(got, rows, refs=[recorded(fx, f"geo_{L}_{hop}_{tag}"), None, None], frame_length=L, hop=hop)


def test_tie_is_inactive_and_one_count_louder_is_active(fx):
    quiet, loud = V.tie_rows()
    got = launch([quiet, loud], threshold=V.TIE_THRESHOLD)
    check(got, [quiet, loud], refs=[recorded(fx, "tie_quiet"), recorded(fx, "tie_loud")])
    assert got["P"][0, 4] == 400.0 and got["P"][0, 14] == 100.0 and got["P"][1, 14] == 121.0
    assert got["active"][0, 14] == 0 and got["active"][1, 14] == 1 and got["active"][:, 4].all()


@pytest.mark.parametrize("min_silence", (1, 2, 3, 8))
def test_fill(fx, min_silence):
    row = V.gaps_row()
    got = launch([row, row[:5000]], min_silence=min_silence)
    check(got, [row, row[:5000]], refs=[recorded(fx, f"fill_{min_silence}"), None], min_silence=min_silence)
    assert got["count"][0] == {1: 6, 2: 5, 3: 4, 8: 2}[min_silence]


def test_margin(fx):
    row = V.speechlike(6000, 23)
    for m in (0, 100, 10 ** 6):
        got = launch([row, row[:2500]], margin=m)
        check(got, [row, row[:2500]], refs=[recorded(fx, f"margin_{m}"), None], margin=m)
    assert got["trim"].tolist() == [[0, 6000], [0, 2500]]  # a margin larger than the row clamps to [0, n]


def test_interval_cap(fx):
    row = V.nine_runs_row()
    ref = recorded(fx, "nine_runs")
    got = launch([row, row[:3000]], max_intervals=4)
    check(got, [row, row[:3000]])
    assert got["count"][0] == 9 and got["intervals"].shape == (2, 4, 2)
    same_bits(got["intervals"][0], ref["iv"][:4])
    assert got["count"][1] < 4 and not got["intervals"][1, got["count"][1]:].any()
    full = launch([row])  # the default cap holds every run
    assert full["count"][0] == 9 and full["intervals"].shape[1] == (V.frames(len(row), 256) + 1) // 2
    same_bits(full["intervals"][0, :9], ref["iv"])
    none = launch([row], max_intervals=0)
    assert none["count"][0] == 9 and none["intervals"].shape == (1, 0, 2)
    same_bits(none["trim"], full["trim"])


def test_layout_independence():
    row = V.speechlike(9001, 51)
    others = [V.speechlike(n, 60 + i) for i, n in enumerate((12000, 1, 700, 0, 5000, 9500))]
    alone = launch([row], min_silence=2)
    first = launch([row] + others, min_silence=2)
    last = launch(others + [row], min_silence=2)
    wide = launch([row], min_silence=2, n_max=20011)
    F = V.frames(len(row), 256)
    for got, b in ((first, 0), (last, 6), (wide, 0)):
        same_bits(got["P"][b, :F], alone["P"][0])
        same_bits(got["Pmax"][b], alone["Pmax"][0])
        same_bits(got["active"][b, :F], alone["active"][0])
        k = alone["count"][0]
        assert got["count"][b] == k
        same_bits(got["intervals"][b, :k], alone["intervals"][0, :k])
        same_bits(got["trim"][b], alone["trim"][0])
        assert (bits(got["P"][b, F:]) == 0).all() and not got["active"][b, F:].any()
    check(first, [row] + others, min_silence=2)
    # a row stride larger than n_max: rows of a wider tensor
    from fs2amd import ops

    wav, lens = V.pack([row] + others, np.int16)
    big = dev(np.concatenate([wav, np.full((7, 33), 77, np.int16)], axis=1))
    P, Pmax, _ = ops.frame_power(big[:, :wav.shape[1]], dev(lens), frame_length=1024, hop_length=256)
    same_bits(P.cpu().numpy(), first["P"])
    same_bits(Pmax.cpu().numpy(), first["Pmax"])


def test_error_returns_leave_the_outputs_untouched():
    """Argument checks only: every call below is refused before anything is launched."""
    from fs2amd import _lib, ops

    lib = _lib.load()
    E, U = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    B, n_max, hop, L = 2, 1000, 256, 1024
    F = V.frames(n_max, hop)
    wav = dev(np.ones((B, n_max), dtype=np.int16))
    gP, gM, gW = Guarded((B, F), torch.float64), Guarded((B,), torch.float64), Guarded((B,), torch.float64)
    gA, gC = Guarded((B, F), torch.uint8), Guarded((B,), torch.int32)
    gI, gT, gR = Guarded((B, 4, 2), torch.int64), Guarded((B, 2), torch.int64), Guarded((B, 10), torch.int16)
    pin = dev(np.ones((B, F))), dev(np.ones(B))
    stream = ops._stream(wav)
    ptr = ops._ptr

    def power(wav_p=ptr(wav), dtype=_lib.FS2_I16, stride=n_max, B=B, n_max=n_max, L=L, hop=hop, P=ptr(gP.view),
              Pmax=ptr(gM.view), ws=ptr(gW.view), ws_bytes=8 * B):
        return lib.fs2_vad_power(wav_p, dtype, stride, None, B, n_max, L, hop, P, Pmax, ws, ws_bytes, stream)

    for kw in (dict(wav_p=None), dict(P=None), dict(Pmax=None), dict(ws=None), dict(B=0), dict(B=-1), dict(n_max=0),
               dict(L=0), dict(hop=0), dict(hop=-3), dict(L=256, hop=257), dict(stride=n_max - 1), dict(ws_bytes=8 * B - 1)):
        assert power(**kw) == E, kw
    for kw in (dict(dtype=_lib.FS2_F64), dict(B=65536), dict(L=4097, hop=1), dict(L=8192, hop=8192),
               dict(n_max=2 ** 31 - 1, stride=2 ** 31 - 1, L=2, hop=1), dict(B=65535, n_max=2 ** 24, stride=2 ** 24)):
        assert power(**kw) == U, kw

    def intervals(P=ptr(pin[0]), Pmax=ptr(pin[1]), B=B, n_max=n_max, hop=hop, thr=0.01, floor=0.1, ms=1, margin=0, cap=4,
                  chunk=0, act=ptr(gA.view), count=ptr(gC.view), iv=ptr(gI.view), trim=ptr(gT.view)):
        return lib.fs2_vad_intervals(P, Pmax, None, B, n_max, hop, thr, floor, ms, margin, cap, chunk, act, count, iv,
                                     trim, stream)

    for kw in (dict(P=None), dict(Pmax=None), dict(act=None), dict(count=None), dict(iv=None), dict(trim=None), dict(B=0),
               dict(n_max=0), dict(hop=0), dict(ms=0), dict(margin=-1), dict(cap=-1), dict(chunk=100),
               dict(thr=-0.5), dict(thr=float("nan")), dict(floor=-1.0)):
        assert intervals(**kw) == E, kw
    for kw in (dict(B=65536), dict(n_max=2 ** 31 - 1, hop=1), dict(B=65535, n_max=2 ** 24), dict(B=65535, cap=2 ** 20)):
        assert intervals(**kw) == U, kw

    def cut(wav_p=ptr(wav), dtype=_lib.FS2_I16, stride=n_max, trim=ptr(gT.view), B=B, n_max=n_max, M=10, out=ptr(gR.view)):
        return lib.fs2_vad_cut(wav_p, dtype, stride, trim, B, n_max, M, out, None, stream)

    for kw in (dict(wav_p=None), dict(trim=None), dict(out=None), dict(B=0), dict(n_max=0), dict(M=0), dict(stride=n_max - 1)):
        assert cut(**kw) == E, kw
    for kw in (dict(dtype=_lib.FS2_BF16), dict(B=65536)):
        assert cut(**kw) == U, kw
    torch.cuda.synchronize()
    for g in (gP, gM, gW, gA, gC, gI, gT, gR):
        assert g.untouched()
    # the wrappers refuse the same things with exceptions
    with pytest.raises(ValueError):
        ops.frame_power(wav, frame_length=256, hop_length=257)
    with pytest.raises(ValueError):
        ops.frame_power(wav, frame_length=4097, hop_length=1)
    with pytest.raises(ValueError):
        ops.activity_intervals(pin[0], pin[1], None, threshold=0.1, floor=0.1, hop_length=hop, min_silence=0)
    with pytest.raises(ValueError):
        ops.activity_intervals(pin[0], pin[1], None, threshold=0.1, floor=0.1, hop_length=hop, n_max=5000)


def test_trim_silence_and_split_silence(fx):
    import fs2amd

    names = ["geo_2048_512_i16", "geo_2048_512_f32", "content_silent", "len_5_0", "len_10_9001", "content_below_floor"]
    cases = V.fixture_cases()
    wavs = [cases[n][0] for n in names]
    refs = [V.analyse(w, frame_length=2048, hop=512) for w in wavs]
    for n, r in zip(names[:2], refs[:2]):  # the recorded tables of the cases the fixture holds at librosa's defaults
        same_bits(r["trim"], fx["trim_" + n])
        same_bits(r["intervals"], fx["iv_" + n])
    cut, se = fs2amd.trim_silence(wavs, device=DEV)
    iv = fs2amd.split_silence(wavs, device=DEV)
    assert se.dtype == np.int64 and se.shape == (len(wavs), 2)
    for b, r in enumerate(refs):
        same_bits(se[b], r["trim"])
        same_bits(cut[b], r["cut"])
        same_bits(iv[b], r["intervals"])
    assert len(cut[3]) == 0 and iv[3].shape == (0, 2)
    order = list(range(len(wavs)))[::-1]  # the opposite order: the same result per utterance
    cut2, se2 = fs2amd.trim_silence([wavs[i] for i in order], device=DEV)
    iv2 = fs2amd.split_silence([wavs[i] for i in order], device=DEV)
    for j, i in enumerate(order):
        same_bits(cut2[j], cut[i])
        same_bits(se2[j], se[i])
        same_bits(iv2[j], iv[i])
    # the other arguments reach the kernels
    w = cases["fill_3"][0]
    r = V.analyse(w, frame_length=1024, hop=256, top_db=40.0, min_silence=3, margin=100)
    cut, se = fs2amd.trim_silence([w], top_db=40.0, frame_length=1024, hop_length=256, min_silence=3, margin=100, device=DEV)
    same_bits(se[0], r["trim"])
    same_bits(cut[0], r["cut"])
    same_bits(fs2amd.split_silence([w], top_db=40.0, frame_length=1024, hop_length=256, min_silence=3, device=DEV)[0],
              fx["iv_fill_3"])
    assert fs2amd.trim_silence([], device=DEV)[0] == [] and fs2amd.split_silence([], device=DEV) == []


def test_prepare_wavs_trims_on_the_device():
    import fs2amd
    import _resample as R

    rfx = R.load_fixture()
    names, ws, _ = R.cases_of(rfx, 441, 320)
    w = ws[names.index("tone_noise")]
    assert w.dtype == np.int16 and len(w) > 2000
    padded = np.concatenate([np.zeros(4000, np.int16), w, np.zeros(5000, np.int16)])
    other = np.concatenate([np.zeros(900, np.int16), ws[names.index("two")], np.zeros(300, np.int16)])
    plain = fs2amd.prepare_wavs([padded, other], 16000, sampling_rate=R.TARGET, device=DEV)
    for kw, akw in ((dict(trim_db=40.0), dict(frame_length=2048, hop=512, top_db=40.0)),
                    (dict(trim_db=30.0, trim_frame_length=1024, trim_hop_length=256, trim_margin=64),
                     dict(frame_length=1024, hop=256, top_db=30.0, margin=64))):
        got = fs2amd.prepare_wavs([padded, other], 16000, sampling_rate=R.TARGET, device=DEV, **kw)
        for g, p in zip(got, plain):
            s, e = V.analyse(p, **akw)["trim"]
            assert g.dtype == np.int16
            same_bits(g, p[s:e])
        assert 0 < len(got[0]) < len(plain[0]) - 8000
    again = fs2amd.prepare_wavs([padded, other], 16000, sampling_rate=R.TARGET, device=DEV, trim_db=None)
    for a, p in zip(again, plain):
        same_bits(a, p)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _same_files(a, b, files):
    match, mismatch, errors = filecmp.cmpfiles(a, b, files, shallow=False)
    assert not mismatch and not errors and len(match) == len(files), (mismatch, errors)


def test_build_corpus_trims_what_brings_no_alignment(tmp_path):
    import fs2amd
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "a"))
    pp = pc["preprocessing"]
    sr, hop, win = pp["audio"]["sampling_rate"], pp["stft"]["hop_length"], pp["stft"]["win_length"]
    assert (hop, win) == (256, 1024)
    utts = _utterances(np.random.default_rng(5))
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    kw = dict(stft=stft, val_size=2, seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)

    # trim_db=None is not passing it
    a, b = str(tmp_path / "plain"), str(tmp_path / "none")
    lines = fs2amd.build_corpus(a, utts, pc, **kw)
    assert fs2amd.build_corpus(b, utts, pc, trim_db=None, trim_margin=0, **kw) == lines and len(lines) == 6
    assert _tree(a) == _tree(b) and len(_tree(a)) > 5
    _same_files(a, b, _tree(a))

    # 0.3 s of zeros (26 hops, so that the frames of the padded recording are those of the bare one, 26 later)
    # around a recording that is silent at its own ends: the cut must be the bare recording's own
    pad = 26 * hop
    assert abs(pad / sr - 0.3) < 0.005
    padded, bare = [], []
    for u in utts:
        w = u["wav"].copy()
        w[:3 * hop + 17] = 0
        w[len(w) - 4 * hop - 5:] = 0
        s, e = V.analyse(w, frame_length=win, hop=hop, top_db=40.0)["trim"]
        assert 0 < s < e < len(w) and s % hop == 0 and e % hop == 0
        frames = int(e - s) // hop
        d = np.full(len(u["phones"]), frames // len(u["phones"]), dtype=np.int64)
        d[-1] += frames - d.sum()
        base = {k: v for k, v in u.items() if k != "f0"}
        long = np.concatenate([np.zeros(pad, np.float32), w, np.zeros(pad, np.float32)])
        sp, ep = V.analyse(long, frame_length=win, hop=hop, top_db=40.0)["trim"]
        assert (sp, ep) == (s + pad, e + pad)
        padded.append(dict(base, wav=long, durations=d))
        bare.append(dict(base, wav=w[s:e], durations=d))
    silent = dict(padded[0], basename="allzero", wav=np.zeros(20000, np.float32), durations=np.array([30, 40]),
                  phones=padded[0]["phones"][:2])
    c, d = str(tmp_path / "trimmed"), str(tmp_path / "bare")
    got = fs2amd.build_corpus(c, padded + [silent], pc, trim_db=40.0, **kw)
    want = fs2amd.build_corpus(d, bare, pc, **kw)
    assert got == want and len(got) >= 4 and not any(m.startswith("allzero|") for m in got)
    files = [f for f in _tree(d) if f.split(os.sep)[0] in ("mel", "energy", "pitch", "duration")]
    assert len(files) == 4 * len(got) and _tree(c) == _tree(d)
    _same_files(c, d, _tree(d))
    # untrimmed, the same utterances give other features: the option did something
    e = str(tmp_path / "untrimmed")
    fs2amd.build_corpus(e, padded, pc, **kw)
    assert filecmp.cmpfiles(c, e, files, shallow=False)[1]
    # durations that cannot fit the trimmed waveform
    bad = dict(padded[1], durations=padded[1]["durations"] + 20)
    with pytest.raises(ValueError, match="trimmed waveform"):
        fs2amd.build_corpus(str(tmp_path / "bad"), [bad], pc, trim_db=40.0, **kw)
    # start / end are cut as before, trim_db or not
    given = [dict({k: v for k, v in u.items() if k != "f0"}, start=0.01, end=0.2) for u in utts[:2]]
    f, g = str(tmp_path / "se"), str(tmp_path / "se_trim")
    short = [dict(u, durations=np.array([4, 6, 5])[:len(u["phones"])], phones=u["phones"][:3]) for u in given]
    assert fs2amd.build_corpus(f, short, pc, **kw) == fs2amd.build_corpus(g, short, pc, trim_db=40.0, **kw)
    _same_files(f, g, _tree(f))
