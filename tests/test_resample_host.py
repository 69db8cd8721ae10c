"""Resampling and peak normalisation, host side (no GPU): the taps against scipy's design, the numpy
restatement of tests/_resample.py against the fixture tests/golden/resample_a.npz and against
scipy.signal.resample_poly itself, the length rule, the int16 rule, and the C ABI of
include/fs2hip_resample.h."""
import os
import re

import numpy as np
import pytest
import torch

import _resample as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_resample.h")


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def test_fixture_has_the_cases_the_kernel_can_get_wrong(fx):
    assert os.path.getsize(os.path.join(R.GOLDEN, "resample_a.npz")) < 400 * 1024
    for up, down in R.RATIOS:
        names, wavs, ys = R.cases_of(fx, up, down)
        lens = [len(w) for w in wavs]
        assert {0, 1, 2, down, down + 1} <= set(lens) and (down - 1 in lens or down == 2) and 3001 in lens
        assert all(w.dtype == np.int16 for w in wavs) and all(y.dtype == np.float64 for y in ys)
        first, last = wavs[names.index(f"impulse_first_{down - 1}")], wavs[names.index(f"impulse_last_{down}")]
        assert first[0] != 0 and not first[1:].any() and last[-1] != 0 and not last[:-1].any()
        assert not wavs[names.index("silence")].any() and len(wavs[names.index("silence")]) > 0
    assert max(len(w) for w in R.cases_of(fx, 441, 320)[1]) > 9000
    twin = fx["wav_441_320"][int(fx["twin"]), :fx["lens32"][0]]
    assert fx["wav32"].dtype == np.float32
    assert (fx["wav32"][0, :fx["lens32"][0]].astype(np.float64) * 32768.0 == twin).all()
    g = fx["wav32"][1, :fx["lens32"][1]].astype(np.float64) * 32768.0
    assert (g != np.round(g)).mean() > 0.9  # the general case is not dyadic


def test_taps_are_scipys_design():
    signal = pytest.importorskip("scipy.signal")
    from fs2amd.audio import resample_taps

    for up, down in R.RATIOS:
        h = resample_taps(up, down)
        half = R.half_len(up, down)
        assert h.dtype == np.float64 and h.shape == (2 * half + 1,)
        same_bits(h, R.taps(up, down))
        ref = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
        err = np.abs(h - ref).max() / np.abs(ref).max()
        print(f"taps {up}/{down}: max |h0 - firwin| / max |firwin| = {err:.2e}")
        assert err <= 2.0 ** -50
        same_bits(h, h[::-1].copy())  # symmetric
        # N roundings of the division (2^-53 |h| each) and a pairwise sum of N terms, sum |h| < 2
        assert np.abs(h).sum() < 2 and abs(h.sum() - 1.0) <= 2.0 ** -48
    with pytest.raises(ValueError):
        resample_taps(0, 3)


def test_ratio_is_the_reduced_fraction():
    from fs2amd.audio import resample_ratio

    for src, want in ((16000, (441, 320)), (48000, (147, 320)), (44100, (1, 2)), (8000, (441, 160)),
                      (24000, (147, 160)), (22050, (1, 1))):
        assert resample_ratio(22050, src) == R.ratio(22050, src) == want
    with pytest.raises(ValueError):
        resample_ratio(22050, 0)


def test_restatement_is_the_fixture(fx):
    for up, down in R.RATIOS:
        h = R.taps(up, down) * up
        for name, w, y in zip(*R.cases_of(fx, up, down)):
            same_bits(R.resample(w, up, down, h), y)
    h = R.taps(441, 320) * 441
    same_bits(R.resample(fx["wav32"][1, :fx["lens32"][1]], 441, 320, h), fx["y_general"])
    t = int(fx["twin"])
    y_twin = R.resample(fx["wav32"][0, :fx["lens32"][0]], 441, 320, h)
    same_bits(y_twin * 32768.0, fx["y_441_320"][t, :len(y_twin)])
    same_bits(R.resample(fx["wav_1_2"][-1], 1, 1, None), fx["wav_1_2"][-1].astype(np.float64))


def test_restatement_is_scipys_resample_poly(fx):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    for up, down in R.RATIOS:
        h0 = R.taps(up, down)
        for n in (0, 1, 2, 319, 320, 321, 1000):
            x = rng.integers(-32768, 32768, n).astype(np.int16)
            same_bits(R.resample(x, up, down, h0 * up), signal.resample_poly(x.astype(np.float64), up, down, window=h0))
        for name, w, y in zip(*R.cases_of(fx, up, down)):
            same_bits(signal.resample_poly(w.astype(np.float64), up, down, window=h0), y)


def test_out_len_is_scipys_output_shape():
    signal = pytest.importorskip("scipy.signal")
    from fs2amd import _lib, ops

    size = _lib.load().fs2_resample_out_len
    for up, down in R.RATIOS:
        h0 = R.taps(up, down)
        for n in range(0, 2001):
            M = signal.resample_poly(np.zeros(n), up, down, window=h0).shape[0]
            assert M == R.out_len(n, up, down) == ops.resample_out_len(n, up, down) == size(n, up, down), (n, up, down)


def test_size_helpers_agree_with_python_integers():
    from fs2amd import _lib

    lib = _lib.load()
    big = 2 ** 31 - 1
    sizes = (1, 2, 3, 147, 160, 319, 320, 321, 441, 496, 497, 65536, big - 1, big)
    for up in sizes:
        for down in sizes:
            for n in (-5, 0, 1, 2, 1000, 5200000, big - 1, big):
                assert lib.fs2_resample_out_len(n, up, down) == R.out_len(n, up, down), (n, up, down)
            N = 20 * max(up, down) + 1
            want = 8 * (N + N // 32 + 1) if max(up, down) <= 1 << 24 else (1 << 63) - 1
            assert lib.fs2_resample_lds_bytes(up, down) == want, (up, down)
    assert lib.fs2_resample_out_len(10, 0, 1) == -1 and lib.fs2_resample_out_len(10, 1, -2) == -1
    assert lib.fs2_resample_lds_bytes(0, 1) == 0 and lib.fs2_resample_lds_bytes(1, 0) == 0
    assert lib.fs2_resample_lds_bytes(441, 320) == 72776 and "441/320: 72776" in open(HEADER).read()
    # the largest ratio term that is staged, and the first that is not
    assert lib.fs2_resample_lds_bytes(496, 1) <= _lib.RESAMPLE_LDS_BYTES < lib.fs2_resample_lds_bytes(497, 1)
    # the ranges of the restatement: inside the utterance and inside the table, for every output
    for up, down in R.RATIOS:
        half = R.half_len(up, down)
        for n in (1, 2, down - 1, down, down + 1, 3001):
            if n < 1:
                continue
            c, lo, hi = R.ranges(n, up, down, half)
            assert (lo >= 0).all() and (hi <= n - 1).all()
            assert (c - lo * up <= 2 * half).all() and (c - hi * up >= 0).all()
            assert ((lo == 0) | (c - (lo - 1) * up > 2 * half)).all() and ((hi == n - 1) | (c - (hi + 1) * up < 0)).all()
            # lo and hi never decrease, and a tile of outputs reads no more samples than the bound
            # the launch sizes its staging with (csrc/resample_sizes.h: rs_span)
            assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all()
            for tile in (1, 7, 2048):
                last = np.minimum(np.arange(len(c)) + tile, len(c)) - 1
                assert (hi[last] - lo + 1).max() <= ((tile - 1) * down + 2 * half) // up + 2


def test_int16_rule_is_numpys_cast_except_at_the_positive_peak(fx):
    seen_peak = 0
    for up, down in R.RATIOS:
        for name, w, y in zip(*R.cases_of(fx, up, down)):
            y32, peak = R.peak_of(y)
            q = R.to_int16(y32, peak)
            assert q.dtype == np.int16 and q.shape == y.shape
            if not peak > 0:
                assert not q.any()
                continue
            v = (y32 / peak) * np.float32(R.MAX_WAV_VALUE)
            ok = v < 32768.0
            same_bits(q[ok], v[ok].astype(np.int16))
            assert (q[~ok] == 32767).all() and (np.abs(q.astype(np.int32)).max() >= 32767)
            seen_peak += int((~ok).sum())
    assert seen_peak > 0  # some case peaks on the positive side
    # the rule itself: toward zero, saturated on both sides
    v = np.array([1.0, 0.99999, -0.99999, -1.0, 0.5 / 32768, -0.5 / 32768, 0.0], dtype=np.float32)
    np.testing.assert_array_equal(R.to_int16(v, np.float32(1.0)), [32767, 32767, -32767, -32768, 0, 0, 0])
    np.testing.assert_array_equal(R.to_int16(v, np.float32(0.5), 65536.0)[:4], [32767, 32767, -32768, -32768])


def test_resample_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_RESAMPLE) == ["fs2_peak_int16", "fs2_resample", "fs2_resample_lds_bytes",
                                                            "fs2_resample_out_len"], declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO)
              | set(_lib.SIGNATURES_AUDIO_INV) | set(_lib.SIGNATURES_PREP) | set(_lib.SIGNATURES_F0))
    assert not set(declared) & others
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_RESAMPLE[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_resample.h" in _lib.EXTRA_HEADERS
    assert re.search(rf"#define FS2_RESAMPLE_LDS_BYTES {_lib.RESAMPLE_LDS_BYTES}\s", open(HEADER).read())


def test_resample_entries_reject_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    P_ = 4096  # a non-NULL pointer that is never dereferenced: every call below returns before a launch
    EINVAL, EUNSUP = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    I16 = _lib.FS2_I16
    #       wav dtype stride lens B n_max up   down taps n_taps y   y32 peak out_lens stream
    good = [P_, I16, 4000, P_, 2, 4000, 441, 320, P_, 8821, P_, P_, P_, P_, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.fs2_resample(*a)

    for k in (0, 8, 11, 12):  # wav, taps, y32, peak
        assert call(**{f"a{k}": None}) == EINVAL, k
    for k in (4, 5, 6, 7):  # B, n_max, up, down
        assert call(**{f"a{k}": 0}) == EINVAL and call(**{f"a{k}": -3}) == EINVAL, k
    assert call(a2=3999) == EINVAL  # stride below the width
    assert call(a9=8820) == EINVAL and call(a9=8822) == EINVAL and call(a9=0) == EINVAL  # not 2 half + 1 taps
    for bad in (_lib.FS2_BF16, _lib.FS2_FP8, _lib.FS2_F64, 9):
        assert call(a1=bad) == EUNSUP
    assert call(a6=497, a7=1, a9=9941) == EUNSUP and call(a6=1, a7=497, a9=9941) == EUNSUP  # beyond the LDS staged
    assert call(a6=2 ** 31 - 1, a7=1, a9=1) == EUNSUP
    assert call(a5=2 ** 31 - 1, a2=2 ** 31 - 1) == EUNSUP  # more than 2^31 - 1 output samples
    # the peak pass
    good_q = [P_, P_, P_, 2, 4000, 32768.0, P_, None]
    for k in (0, 1, 6):
        a = list(good_q)
        a[k] = None
        assert lib.fs2_peak_int16(*a) == EINVAL
    for k in (3, 4):
        a = list(good_q)
        a[k] = 0
        assert lib.fs2_peak_int16(*a) == EINVAL
    a = list(good_q)
    a[3] = 65536
    assert lib.fs2_peak_int16(*a) == EUNSUP


def test_resample_api_is_exported_and_refuses_cpu_tensors():
    import fs2amd
    import fs2amd.library as lib
    from fs2amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert hasattr(fs2amd, "prepare_wavs") and "prepare_wavs" in fs2amd.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample(torch.zeros(2, 4000, dtype=torch.int16), up=441, down=320, taps=torch.zeros(8821, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.peak_int16(torch.zeros(2, 40), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.prepare_wavs([np.zeros(100, dtype=np.int16)], [16000], sampling_rate=22050, device="cpu")
    with pytest.raises(ValueError):
        fs2amd.prepare_wavs([np.zeros(100, dtype=np.float64)], [16000], sampling_rate=22050, device="cuda")
    assert lib.OPS_RESAMPLE == ("resample", "peak_int16") and all(hasattr(torch.ops.fs2, n) for n in lib.OPS_RESAMPLE)
    assert not set(lib.OPS_RESAMPLE) & (set(lib.OPS) | set(lib.OPS_PREP) | set(lib.OPS_F0))
    with FakeTensorMode():
        wav = torch.empty(3, 5000, device="cuda", dtype=torch.int16)
        taps = torch.empty(8821, device="cuda", dtype=torch.float64)
        y, y32, peak, out_lens = torch.ops.fs2.resample(wav, None, taps, 441, 320)
        assert y.shape == y32.shape == (3, R.out_len(5000, 441, 320)) and peak.shape == out_lens.shape == (3,)
        assert (y.dtype, y32.dtype, peak.dtype, out_lens.dtype) == (torch.float64, torch.float32, torch.float32, torch.int64)
        q = torch.ops.fs2.peak_int16(y32, peak, out_lens, 32768.0)
        assert q.shape == y32.shape and q.dtype == torch.int16
