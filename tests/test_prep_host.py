"""Corpus preprocessing, host side (no GPU): the numpy restatement of tests/_prep.py against every
output of the reference stored in tests/golden/prep_a.npz, get_alignment, and the C ABI of
include/fs2hip_prep.h."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _prep as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_prep.h")
ENTRY_POINTS = ["fs2_moments_merge", "fs2_normalize_minmax", "fs2_normalize_minmax_ws_bytes", "fs2_outlier_moments",
                "fs2_pitch_targets"]


@pytest.fixture(scope="module")
def fx():
    return P.load_fixture()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_fixture_has_the_cases_the_kernels_can_get_wrong(fx):
    lens = list(fx["f0_lens"])
    assert set([1, 2, 63, 64, 65, 129, 300, 700]) <= set(lens)
    assert list(fx["track_lens"][:14]) == [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 2049]
    names = list(fx["pitch_names"])
    dropped = [i for i, n in enumerate(names) if "dropped" in n]
    assert len(dropped) == 3 and sorted(fx["ref_voiced"][dropped]) == [0, 1, 1] and (fx["ref_filled_lens"][dropped] == 0).all()
    assert 2 in fx["ref_voiced"] and (fx["ref_voiced"] == fx["f0_lens"]).any()  # exactly two voiced; fully voiced
    for f0, d in zip(P.ragged(fx, "f0", "f0_lens"), P.ragged(fx, "dur", "dur_lens")):
        assert all(d[:i].sum() >= i for i in range(len(d))) and d.sum() <= len(f0)
    assert any((d[1:] == 0).any() for d in P.ragged(fx, "dur", "dur_lens"))
    assert fx["tracks64"].dtype == np.float64 and fx["tracks32"].dtype == np.float32
    rep = P.ragged(fx, "tracks64", "track_lens")[14]
    assert len(np.unique(rep)) < len(rep) // 2  # repeated values


def test_pitch_restatement_equals_the_reference(fx):
    f0s, durs = P.ragged(fx, "f0", "f0_lens"), P.ragged(fx, "dur", "dur_lens")
    filled, ph = P.ragged(fx, "ref_filled", "ref_filled_lens"), P.ragged(fx, "ref_ph", "ref_ph_lens")
    for b, (f0, d) in enumerate(zip(f0s, durs)):
        r_ph, r_filled, voiced = P.pitch_target(f0, d)
        assert voiced == fx["ref_voiced"][b]
        if voiced <= 1:
            assert r_ph is None and r_filled is None and len(filled[b]) == 0 and len(ph[b]) == 0
            continue
        np.testing.assert_array_equal(bits(r_filled), bits(filled[b]))  # bit for bit
        assert len(r_filled) == min(len(f0), d.sum())
        assert (np.abs(r_ph - ph[b]) <= P.mean_bounds(filled[b], d)).all()
        assert (ph[b][d == 0] == 0).all()
        # a voiced frame that is not the first goes through the formula: not always the input's bits
        ids = np.where(f0[:d.sum()] != 0)[0]
        np.testing.assert_allclose(r_filled[ids], f0[ids], rtol=1e-15, atol=0)
        assert r_filled[ids[0]] == f0[ids[0]] and (r_filled[:ids[0]] == f0[ids[0]]).all()
        assert (r_filled[ids[-1] + 1:] == f0[ids[-1]]).all()


@pytest.mark.parametrize("tag", ["64", "32"])
def test_fence_restatement_equals_the_reference(fx, tag):
    tracks, masks = P.ragged(fx, f"tracks{tag}", "track_lens"), P.ragged(fx, f"mask{tag}", "track_lens")
    for i, v in enumerate(tracks):
        mask, p25, p75 = P.outlier_fence(v)
        np.testing.assert_array_equal(mask, masks[i])
        q = np.array([p25, p75], dtype=v.dtype)
        assert q.dtype == fx[f"quart{tag}"].dtype
        np.testing.assert_array_equal(bits(q), bits(fx[f"quart{tag}"][i]))
    assert np.isnan(fx[f"quart{tag}"][0]).all() and not masks[1].any()  # n = 0, n = 1
    if tag == "32":  # the element on the upper fence is out
        v, m = tracks[-1], masks[-1]
        assert tuple(fx["quart32"][-1]) == (2.0, 6.0) and not m[v == 12.0].any() and m.sum() == len(v) - 1


def test_normalize_restatement_equals_the_reference(fx):
    ids = fx["norm_ids"]
    for tag, key, mean, std in (("64", "tracks64", fx["scaler64_mean"][-1], fx["scaler64_scale"]),
                                ("32", "tracks32", fx["scaler32_mean"][-1], fx["scaler32_scale"]),
                                ("32_off", "tracks32", 0, 1)):
        tracks = [P.ragged(fx, key, "track_lens")[i] for i in ids]
        vals, vmin, vmax = P.normalize(tracks, mean[()] if tag != "32_off" else 0, std[()] if tag != "32_off" else 1)
        got = np.concatenate(vals)
        assert got.dtype == fx[f"norm{tag}"].dtype == (np.float32 if tag == "32_off" else np.float64)
        np.testing.assert_array_equal(bits(got), bits(fx[f"norm{tag}"]))
        assert (vmin, vmax) == tuple(fx[f"norm{tag}_minmax"])


def test_reference_scaler_is_within_the_updating_bound(fx):
    for tag in ("64", "32"):
        ex = P.ExactMoments()
        for i, v in enumerate(P.ragged(fx, f"tracks{tag}", "track_lens")):
            kept = v[P.outlier_fence(v)[0]]
            ex.add(kept)
            assert ex.n == fx[f"scaler{tag}_n"][i]
            if ex.n:
                r = ex.ratios(fx[f"scaler{tag}_mean"][i], fx[f"scaler{tag}_var"][i])
                assert max(r) <= 1.0, (tag, i, r)
        assert fx[f"scaler{tag}_scale"] == np.sqrt(fx[f"scaler{tag}_var"][-1])


def test_get_alignment():
    from fs2amd.preprocess import get_alignment

    sr, hop = 22050, 256
    tier = [(0.0, 0.31, "sil"), (0.31, 0.5, "n"), (0.5, 0.9, "i"), (0.9, 1.0, "sp"), (1.0, 1.37, "h"), (1.37, 1.8, "ao"),
            (1.8, 2.1, "sp"), (2.1, 2.5, "sil")]
    phones, dur, start, end = get_alignment(tier, sr, hop)
    assert phones == ["n", "i", "sp", "h", "ao"] and (start, end) == (0.31, 1.8)
    fr = [int(np.round(e * sr / hop) - np.round(s * sr / hop)) for s, e, _ in tier[1:6]]
    assert dur == fr and all(isinstance(d, int) for d in dur)
    assert sum(dur) == int(np.round(1.8 * sr / hop) - np.round(0.31 * sr / hop))
    # leading "sp" and "spn" are silences too; a tier without a trailing silence ends at its last phone
    phones, dur, start, end = get_alignment([(0.0, 0.1, "sp"), (0.1, 0.2, "spn"), (0.2, 0.45, "a")], sr, hop)
    assert phones == ["a"] and (start, end) == (0.2, 0.45) and dur == [22]
    # nothing but silence: start >= end, the caller drops the utterance
    phones, dur, start, end = get_alignment([(0.0, 0.4, "sil"), (0.4, 0.9, "sp")], sr, hop)
    assert phones == [] and dur == [] and start >= end
    assert get_alignment([], sr, hop) == ([], [], 0, 0)


def test_prep_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_PREP) == ENTRY_POINTS, declared
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO)
                                | set(_lib.SIGNATURES_AUDIO_INV))
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_PREP[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_prep.h" in _lib.EXTRA_HEADERS  # the build id covers the header
    assert _lib.FS2_F64 == 4 and _lib.FS2_I16 == 3 and (_lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_FP8) == (0, 1, 2)
    text = open(HEADER).read()
    for name, val in (("FS2_F64", _lib.FS2_F64), ("FS2_PITCH_T_MAX", _lib.PITCH_T_MAX),
                      ("FS2_PITCH_T_MAX_NOFILL", _lib.PITCH_T_MAX_NOFILL), ("FS2_OUTLIER_LDS_BYTES", _lib.OUTLIER_LDS_BYTES)):
        assert f"#define {name} {val} " in text or f"#define {name} {val}\n" in text, name


def test_prep_entries_reject_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    P_ = 4096  # a non-NULL pointer that is never dereferenced: every call below returns before a launch
    EINVAL, EUNSUP = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    pt = lib.fs2_pitch_targets
    assert pt(None, 8, None, P_, 1, 8, 2, P_, P_, P_, None) == EINVAL
    assert pt(P_, 8, None, None, 1, 8, 2, P_, P_, P_, None) == EINVAL
    assert pt(P_, 8, None, P_, 1, 8, 2, None, P_, P_, None) == EINVAL
    assert pt(P_, 8, None, P_, 1, 8, 2, P_, P_, None, None) == EINVAL
    assert pt(P_, 8, None, P_, 0, 8, 2, P_, P_, P_, None) == EINVAL
    assert pt(P_, 8, None, P_, 1, 0, 2, P_, P_, P_, None) == EINVAL
    assert pt(P_, 8, None, P_, 1, 8, 0, P_, P_, P_, None) == EINVAL
    assert pt(P_, 7, None, P_, 1, 8, 2, P_, P_, P_, None) == EINVAL  # stride below the width
    assert pt(P_, 1 << 20, None, P_, 1, _lib.PITCH_T_MAX + 1, 2, P_, P_, P_, None) == EUNSUP
    assert pt(P_, 1 << 20, None, P_, 1, _lib.PITCH_T_MAX_NOFILL + 1, 2, P_, None, P_, None) == EUNSUP

    om = lib.fs2_outlier_moments
    F32, F64 = _lib.FS2_F32, _lib.FS2_F64
    good = [P_, F64, 16, P_, 2, 16, P_, P_, P_, P_, P_, None]
    for k in (0, 6, 7, 8, 9, 10):  # every required pointer
        a = list(good)
        a[k] = None
        assert om(*a) == EINVAL, k
    assert om(P_, F64, 16, P_, 0, 16, P_, P_, P_, P_, P_, None) == EINVAL
    assert om(P_, F64, 16, P_, 2, 0, P_, P_, P_, P_, P_, None) == EINVAL
    assert om(P_, F64, 15, P_, 2, 16, P_, P_, P_, P_, P_, None) == EINVAL
    for bad in (_lib.FS2_BF16, _lib.FS2_FP8, _lib.FS2_I16, 5):
        assert om(P_, bad, 16, P_, 2, 16, P_, P_, P_, P_, P_, None) == EUNSUP
    assert om(P_, F64, 8193, P_, 2, 8193, P_, P_, P_, P_, P_, None) == EUNSUP  # 64 KB of LDS sorts 8192 f64
    assert om(P_, F32, 16385, P_, 2, 16385, P_, P_, P_, P_, P_, None) == EUNSUP

    mm = lib.fs2_moments_merge
    for k in range(3):
        a = [P_, P_, P_, 4, P_, None]
        a[k] = None
        assert mm(*a) == EINVAL
    assert mm(P_, P_, P_, 4, None, None) == EINVAL and mm(P_, P_, P_, 0, P_, None) == EINVAL

    nm = lib.fs2_normalize_minmax
    assert lib.fs2_normalize_minmax_ws_bytes(0) == 0 and lib.fs2_normalize_minmax_ws_bytes(5) == 80
    good = [P_, F32, 16, P_, 5, 16, 0.0, 1.0, P_, P_, P_, 80, None]
    for k in (0, 8, 9, 10):
        a = list(good)
        a[k] = None
        assert nm(*a) == EINVAL, k
    for k, v in ((4, 0), (5, 0), (2, 15), (11, 79)):  # B, n_max, the stride, the workspace
        a = list(good)
        a[k] = v
        assert nm(*a) == EINVAL, k
    for bad in (_lib.FS2_BF16, _lib.FS2_I16, 7):
        a = list(good)
        a[1] = bad
        assert nm(*a) == EUNSUP


def test_prep_api_is_exported_and_refuses_cpu_tensors():
    import fs2amd
    from fs2amd import ops

    for name in ("get_alignment", "pitch_targets", "remove_outlier", "CorpusStats", "normalize", "build_corpus"):
        assert hasattr(fs2amd, name) and name in fs2amd.__all__
    f0, dur = torch.zeros(2, 8, dtype=torch.float64), torch.ones(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pitch_targets(f0, dur)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.outlier_moments(torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normalize_minmax(torch.zeros(2, 8), mean=0.0, std=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moments_merge(torch.zeros(3, dtype=torch.float64), torch.zeros(2, dtype=torch.int64),
                          torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.CorpusStats(device="cpu")
    import fs2amd.library as lib
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert all(hasattr(torch.ops.fs2, n) for n in lib.OPS_PREP)
    with FakeTensorMode():
        f0 = torch.empty(3, 50, device="cuda", dtype=torch.float64)
        out, filled, voiced = torch.ops.fs2.pitch_targets(f0, torch.empty(3, 7, device="cuda", dtype=torch.int64), None)
        assert out.shape == (3, 7) and filled.shape == (3, 50) and voiced.shape == (3,) and voiced.dtype == torch.int32
        assert out.dtype == filled.dtype == torch.float64
        v = torch.empty(3, 40, device="cuda", dtype=torch.float32)
        q, inl, cnt, mean, m2 = torch.ops.fs2.outlier_moments(v, None)
        assert q.shape == (3, 2) and q.dtype == torch.float32 and inl.shape == (3, 40) and inl.dtype == torch.bool
        assert cnt.dtype == torch.int64 and mean.dtype == m2.dtype == torch.float64 and mean.shape == (3,)
        o, mm = torch.ops.fs2.normalize_minmax(v, None, 1.0, 2.0)
        assert o.shape == (3, 40) and o.dtype == torch.float64 and mm.shape == (2,)
