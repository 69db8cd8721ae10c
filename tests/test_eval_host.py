"""Objective evaluation, host side (no GPU): the numpy restatements of tests/_eval.py against a
brute-force enumeration of every warping path, the tie rule, scipy's DCT (tests/golden/eval_a.npz),
and the C ABI and size helper of include/fs2hip_eval.h."""
import importlib
import os
import re
import shutil

import numpy as np
import pytest
import torch

import _eval as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_eval.h")
U = 2.0 ** -52


@pytest.fixture(scope="module")
def fx():
    return E.load_golden()


def test_fixture_is_the_case_table(fx):
    assert [tuple(c) for c in fx["cases"]] == list(E.CASES)
    assert os.path.getsize(E.GOLDEN) < 1 << 20
    _, _, xs, ys = E.batch_feats(np.float64)
    for b, (Tx, Ty) in enumerate(E.CASES):
        assert fx[f"x{b}"].shape == (Tx, E.D) and fx[f"y{b}"].shape == (Ty, E.D) and fx[f"x{b}"].dtype == np.float64
        np.testing.assert_array_equal(fx[f"x{b}"], xs[b])
        np.testing.assert_array_equal(fx[f"y{b}"], ys[b])
        for tag, K in (("", fx["K"][b]), ("32_", fx["K32"][b])):
            pi, pj = fx[f"pi{tag}{b}"], fx[f"pj{tag}{b}"]
            assert pi.dtype == np.int32 and pi.shape == pj.shape == (K,) and max(Tx, Ty) <= K <= Tx + Ty - 1
            assert (pi[0], pj[0]) == (0, 0) and (pi[-1], pj[-1]) == (Tx - 1, Ty - 1)
            di, dj = np.diff(pi), np.diff(pj)
            assert ((di >= 0) & (di <= 1) & (dj >= 0) & (dj <= 1) & (di + dj >= 1)).all()
    assert max(Tx for Tx, _ in E.CASES) <= E.TX_MAX and max(Ty for _, Ty in E.CASES) <= E.TY_MAX
    assert np.isfinite(fx["total"]).all() and (fx["total"] > 0).all()
    # the recursion written a second time, row by row with Python floats: the same bits
    np.testing.assert_array_equal(fx["total"].view(np.uint64), fx["total_rowwise"].view(np.uint64))


def test_restatement_is_the_best_warping_path():
    """Every warping path of every (Tx, Ty) <= (5, 5): the totals agree within 1e-12 (the recursion
    adds the end cell last, the enumeration the start cell first) and the path is among the best."""
    rng = np.random.default_rng(3)
    for Tx in range(1, 6):
        for Ty in range(1, 6):
            for trial in range(3):
                x = E.make_feats(Tx, 3, 50 * Tx + 7 * Ty + trial) if trial else rng.standard_normal((Tx, 3))
                y = E.make_feats(Ty, 3, 900 + 50 * Tx + 7 * Ty + trial)
                c = E.pair_dist_ref(x, y)
                total, K, pi, pj = E.dtw_ref(x, y)
                best, arg = E.dtw_brute(c)
                assert abs(total - best) <= 1e-12, (Tx, Ty, trial, total, best)
                assert tuple(zip(pi.tolist(), pj.tolist())) in arg, (Tx, Ty, trial)
                assert max(Tx, Ty) <= K <= Tx + Ty - 1


def test_tie_rule_and_hand_built_path():
    def path(x, y):
        total, K, pi, pj = E.dtw_ref(np.asarray(x, dtype=np.float64)[:, None], np.asarray(y, dtype=np.float64)[:, None])
        return total, list(zip(pi.tolist(), pj.tolist()))

    # constant sequences: every cost ties; the diagonal first, then up (i - 1) before left (j - 1)
    assert path([2.0] * 5, [2.0] * 3) == (0.0, [(0, 0), (1, 0), (2, 0), (3, 1), (4, 2)])
    assert path([2.0] * 3, [2.0] * 5) == (0.0, [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)])
    # D = 1: the distances are perfect squares' roots, the total exact
    assert path([0, 3, 7, 7, 12], [1, 7, 13]) == (4.0, [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)])


def test_cepstrum_restatement_agrees_with_scipy_dct(fx):
    """c = mel . basis^T summed in index order against scipy.fft.dct(type=2, norm="ortho")[:, 1:14]:
    atol M u sum_m |mel[t, m] basis[q, m]| with u = 2^-52, M = 80: the rounding-error bound of an
    80-term sum at unit roundoff 2^-53, doubled for scipy's own error and the table's rounding."""
    mel, want = fx["mel"], fx["dct_scipy"]
    basis = E.dct_basis()
    assert basis.shape == (E.N_COEF, E.N_MEL) and want.shape == (mel.shape[0], E.N_COEF)
    got = E.mel_cepstrum_ref(mel, basis)
    bound = E.N_MEL * U * (np.abs(mel)[:, None, :] * np.abs(basis)[None, :, :]).sum(-1)
    ratio = np.abs(got - want) / bound
    print(f"cepstrum restatement against scipy: worst error {ratio.max() * E.N_MEL:.2f} u sum|terms| (bound {E.N_MEL})")
    assert (ratio <= 1.0).all(), ratio.max()
    # orthonormal rows, and the module's table is the restatement's
    np.testing.assert_allclose(basis @ basis.T, np.eye(E.N_COEF), atol=1e-14)
    ev = importlib.import_module("fs2amd.evaluate")
    np.testing.assert_array_equal(ev.dct_basis(E.N_MEL, E.N_COEF), basis)
    assert ev.ALPHA == E.ALPHA == 10.0 / np.log(10.0) * np.sqrt(2.0)
    with pytest.raises(ValueError):
        ev.dct_basis(13, 13)


def test_path_stats_restatement_counts_and_sums():
    a = np.array([[1.0], [np.nan], [4.0], [np.nan]])
    b = np.array([[0.5], [2.0], [np.nan]])
    pi, pj = np.array([0, 1, 2, 3, 3]), np.array([0, 0, 1, 1, 2])
    counts, sums = E.path_stats_ref(a, b, pi, pj, 5)
    assert counts.tolist() == [[2, 0, 2, 1]] and sums.tolist() == [[0.5 + 2.0, 0.25 + 4.0]]
    counts, sums = E.path_stats_ref(a, b, pi, pj, 0)
    assert not counts.any() and not sums.any()
    t = E.f0_tracks(np.array([0.0, 220.0, 440.0]))
    assert np.isnan(t[0]).all() and t[1, 0] == 220.0 and abs((t[2, 1] - t[1, 1]) - 1200.0) < 1e-9


def test_eval_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_EVAL) == ["fs2_dtw", "fs2_dtw_lds_bytes", "fs2_dtw_ws_bytes",
                                                        "fs2_mel_cepstrum", "fs2_pair_dist", "fs2_path_stats"], declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO)
              | set(_lib.SIGNATURES_AUDIO_INV) | set(_lib.SIGNATURES_PREP) | set(_lib.SIGNATURES_F0)
              | set(_lib.SIGNATURES_RESAMPLE) | set(_lib.SIGNATURES_ALIGN))
    assert not set(declared) & others
    assert len(_lib.header_symbols(_lib.HEADER)) == 71  # fs2hip.h stays as it was
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_EVAL[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_eval.h" in _lib.EXTRA_HEADERS and _lib.HEADER_EVAL == HEADER
    text = open(HEADER).read()
    for name, val in (("FS2_DTW_LDS_BYTES", _lib.DTW_LDS_BYTES), ("FS2_DTW_LDS_SMALL", _lib.DTW_LDS_SMALL),
                      ("FS2_DTW_AUTO", _lib.DTW_AUTO), ("FS2_DTW_LDS", _lib.DTW_LDS), ("FS2_DTW_GLOBAL", _lib.DTW_GLOBAL)):
        assert re.search(rf"#define {name} {val}\s", text), name
    sizes = open(os.path.join(REPO, "expressive-fastspeech2-mandarin_amd", "csrc", "eval_sizes.h")).read()
    assert re.search(r"#define FS2_EV_SIZE_CAP \(1 << 24\)", sizes) and _lib.EVAL_SIZE_CAP == 1 << 24


def test_size_mirror_agrees_with_the_library():
    from fs2amd import _lib

    lib = _lib.load()
    big = (1 << 31) - 1
    sizes = (-1, 0, 1, 2, 63, 64, 65, 130, 270, 300, 520, 524, 529, 530, 700, 860, 2000, 6823, 6824, 1 << 24,
             (1 << 24) + 1, big)
    for Tx in sizes:
        for Ty in sizes:
            for in_lds in (0, 1):
                assert lib.fs2_dtw_lds_bytes(Tx, Ty, in_lds) == _lib.dtw_lds_bytes(Tx, Ty, bool(in_lds)), (Tx, Ty, in_lds)
            for B in (0, 1, 64, big):
                assert lib.fs2_dtw_ws_bytes(B, Tx, Ty) == _lib.dtw_ws_bytes(B, Tx, Ty), (B, Tx, Ty)
    # the sizes the documents quote
    assert _lib.dtw_lds_bytes(524, 520) == 8 * (3 * 527 + 1043 * 2 * 9) == 162840 <= _lib.DTW_LDS_BYTES
    assert _lib.dtw_form(524, 520) == (_lib.FS2_OK, _lib.DTW_LDS) and _lib.dtw_form(529, 520)[1] == _lib.DTW_LDS
    assert _lib.dtw_form(530, 520) == (_lib.FS2_OK, _lib.DTW_GLOBAL)  # the first Tx past the LDS at Ty = 520
    assert _lib.dtw_lds_bytes(860, 860) == 8 * (3 * 863 + 1719 * 2 * 14) == 405768 > _lib.DTW_LDS_BYTES
    assert 860 * 860 * 2 // 8 > _lib.DTW_LDS_BYTES  # no 2-bit layout puts 860 x 860 in LDS
    assert _lib.dtw_lds_bytes(860, 860, False) == 20712 <= _lib.DTW_LDS_SMALL
    assert _lib.dtw_ws_bytes(64, 860, 860) == 64 * 1719 * 2 * 14 * 8 == 24643584
    assert _lib.dtw_form(860, 860) == (_lib.FS2_OK, _lib.DTW_GLOBAL)
    assert _lib.dtw_form(860, 860, _lib.DTW_LDS) == (_lib.FS2_EUNSUPPORTED, None)
    assert _lib.dtw_form(2000, 700) == (_lib.FS2_OK, _lib.DTW_GLOBAL) and _lib.dtw_lds_bytes(2000, 700, False) > _lib.DTW_LDS_SMALL
    assert _lib.dtw_lds_bytes(300, 270) == 52792 and _lib.dtw_form(300, 270) == (_lib.FS2_OK, _lib.DTW_LDS)
    assert _lib.dtw_form(6823, 5) == (_lib.FS2_OK, _lib.DTW_GLOBAL) and _lib.dtw_form(6824, 5)[0] == _lib.FS2_EUNSUPPORTED


def test_size_mirror_agrees_with_the_standalone_check():
    """tools/eval_sizes_check.py: the stand-alone host program over csrc/eval_sizes.h prints what the
    Python mirror gives at every boundary size. The tool's own run builds it with ASan and UBSan (DESIGN
    9.6 records that run); here the same program is built plainly, so that the comparison does not
    depend on a sanitizer runtime where the suite runs."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("eval_sizes_check", os.path.join(REPO, "tools", "eval_sizes_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cxx = shutil.which("g++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler build() uses otherwise
    assert mod.check(cxx, sanitize=False) > 5000


def test_eval_entries_reject_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    P_ = 4096  # a non-NULL pointer that is never dereferenced: every call below returns before a launch
    EINVAL, EUNSUP = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED

    def call(fn, base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)

    #      mel dtype        bs        rs  lens basis B  T    M   C   out stream
    cep = [P_, _lib.FS2_F32, 100 * 80, 80, P_, P_, 4, 100, 80, 13, P_, None]
    f = lib.fs2_mel_cepstrum
    for k in (0, 5, 10):
        assert call(f, cep, **{f"a{k}": None}) == EINVAL, k
    for k in (6, 7, 8, 9):
        assert call(f, cep, **{f"a{k}": 0}) == EINVAL and call(f, cep, **{f"a{k}": -3}) == EINVAL, k
    assert call(f, cep, a3=79) == EINVAL and call(f, cep, a2=99 * 80 + 79) == EINVAL  # overlapping rows
    assert call(f, cep, a6=1 << 20, a7=1 << 10, a2=(1 << 10) * 80) == EINVAL  # more than 2^31 - 1 outputs
    for bad in (_lib.FS2_BF16, _lib.FS2_FP8, _lib.FS2_I16, 9):
        assert call(f, cep, a1=bad) == EUNSUP
    #      x   y   dtype         xbs       xrs ybs      yrs xl  yl  B  Tx   Ty  D   sq out stream
    pd = [P_, P_, _lib.FS2_F64, 100 * 13, 13, 90 * 13, 13, P_, P_, 4, 100, 90, 13, 0, P_, None]
    f = lib.fs2_pair_dist
    for k in (0, 1, 14):
        assert call(f, pd, **{f"a{k}": None}) == EINVAL, k
    for k in (9, 10, 11, 12):
        assert call(f, pd, **{f"a{k}": 0}) == EINVAL and call(f, pd, **{f"a{k}": -1}) == EINVAL, k
    assert call(f, pd, a4=12) == EINVAL and call(f, pd, a6=12) == EINVAL
    assert call(f, pd, a3=99 * 13 + 12) == EINVAL and call(f, pd, a5=89 * 13 + 12) == EINVAL
    assert call(f, pd, a9=1, a10=65536, a11=65536) == EINVAL  # more than 2^31 - 1 outputs
    assert call(f, pd, a2=_lib.FS2_BF16) == EUNSUP and call(f, pd, a2=7) == EUNSUP
    #       x   y   dtype         xbs       xrs ybs      yrs xl  yl  B  Tx   Ty  D   bm ws    wsb tot K   pi  pj  stream
    dtw = [P_, P_, _lib.FS2_F32, 100 * 13, 13, 90 * 13, 13, P_, P_, 4, 100, 90, 13, 0, None, 0, P_, P_, P_, P_, None]
    f = lib.fs2_dtw
    for k in (0, 1, 16, 17, 18, 19):
        assert call(f, dtw, **{f"a{k}": None}) == EINVAL, k
    for k in (9, 10, 11, 12):
        assert call(f, dtw, **{f"a{k}": 0}) == EINVAL and call(f, dtw, **{f"a{k}": -1}) == EINVAL, k
    assert call(f, dtw, a4=12) == EINVAL and call(f, dtw, a5=89 * 13 + 12) == EINVAL
    assert call(f, dtw, a13=3) == EINVAL and call(f, dtw, a13=-1) == EINVAL
    assert call(f, dtw, a13=_lib.DTW_GLOBAL) == EINVAL  # no workspace
    assert call(f, dtw, a13=_lib.DTW_GLOBAL, a14=P_, a15=_lib.dtw_ws_bytes(4, 100, 90) - 1) == EINVAL
    for bad in (_lib.FS2_BF16, _lib.FS2_FP8, _lib.FS2_I16, 9):
        assert call(f, dtw, a2=bad) == EUNSUP
    wide = dict(a10=860, a11=860, a3=860 * 13, a5=860 * 13)
    assert call(f, dtw, a13=_lib.DTW_LDS, **wide) == EUNSUP
    assert call(f, dtw, **wide) == EINVAL  # auto -> global: no workspace
    assert call(f, dtw, a10=6824, a3=6824 * 13, a14=P_, a15=1 << 40) == EUNSUP  # the rows alone
    #     a   b   pi  pj  K   B  Tx   Ty  Ch cnt sums stream
    ps = [P_, P_, P_, P_, P_, 4, 100, 90, 2, P_, P_, None]
    f = lib.fs2_path_stats
    for k in (0, 1, 2, 3, 4, 9, 10):
        assert call(f, ps, **{f"a{k}": None}) == EINVAL, k
    for k in (5, 6, 7, 8):
        assert call(f, ps, **{f"a{k}": 0}) == EINVAL, k


def test_eval_api_is_exported_and_refuses_cpu_tensors():
    import fs2amd
    import fs2amd.library as lib
    from fs2amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode

    ev = importlib.import_module("fs2amd.evaluate")
    for name in ("mcd", "dtw", "mel_cepstrum", "f0_metrics", "evaluate"):
        assert getattr(fs2amd, name) is getattr(ev, name) and name in fs2amd.__all__
    assert fs2amd.__all__[-5:] == ["mcd", "dtw", "mel_cepstrum", "f0_metrics", "evaluate"]
    x, y = torch.zeros(2, 6, 13), torch.zeros(2, 5, 13)
    mel = torch.zeros(2, 6, 80)
    refused = pytest.raises(RuntimeError, match="no CPU fallback")
    with refused:
        ops.mel_cepstrum(mel, [6, 6], basis=torch.zeros(13, 80, dtype=torch.float64))
    with refused:
        ops.pair_dist(x, [6, 6], y, [5, 5])
    with refused:
        ops.dtw(x, [6, 6], y, [5, 5])
    with refused:
        ops.path_stats(x.double(), y.double(), torch.zeros(2, 10, dtype=torch.int32), torch.zeros(2, 10, dtype=torch.int32),
                       torch.zeros(2, dtype=torch.int32))
    with refused:
        fs2amd.mcd(mel, [6, 6], mel, [6, 6])
    with refused:
        fs2amd.mel_cepstrum(mel, [6, 6])
    with refused:
        fs2amd.f0_metrics(torch.zeros(2, 6), torch.zeros(2, 5), None)
    assert lib.OPS_EVAL == ("mel_cepstrum", "pair_dist", "dtw", "path_stats") and all(hasattr(torch.ops.fs2, n) for n in lib.OPS_EVAL)
    assert not set(lib.OPS_EVAL) & (set(lib.OPS) | set(lib.OPS_PREP) | set(lib.OPS_F0) | set(lib.OPS_RESAMPLE)
                                    | set(lib.OPS_ALIGN))
    for op in lib.OPS_EVAL:
        assert f"fs2::{op}" in lib.__doc__
    with FakeTensorMode():
        mel = torch.empty(3, 50, 80, device="cuda")
        c = torch.ops.fs2.mel_cepstrum(mel, None, torch.empty(13, 80, device="cuda", dtype=torch.float64))
        assert c.shape == (3, 50, 13) and c.dtype == torch.float64
        x, y = torch.empty(3, 50, 13, device="cuda"), torch.empty(3, 41, 13, device="cuda")
        cost = torch.ops.fs2.pair_dist(x, None, y, None)
        assert cost.shape == (3, 50, 41) and cost.dtype == torch.float64
        total, K, pi, pj = torch.ops.fs2.dtw(x, None, y, None, 0)
        assert total.shape == (3,) and total.dtype == torch.float64 and K.shape == (3,) and K.dtype == torch.int32
        assert pi.shape == pj.shape == (3, 90) and pi.dtype == pj.dtype == torch.int32
        a, b = torch.empty(3, 50, 2, device="cuda", dtype=torch.float64), torch.empty(3, 41, 2, device="cuda", dtype=torch.float64)
        counts, sums = torch.ops.fs2.path_stats(a, b, pi, pj, K)
        assert counts.shape == (3, 2, 4) and counts.dtype == torch.int64 and sums.shape == (3, 2, 2) and sums.dtype == torch.float64
