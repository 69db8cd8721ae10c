"""Alignment, host side (no GPU): the numpy restatements of tests/_align.py against torch's CPU
float64 ctc_loss (tests/golden/align_a.npz) and against a brute-force enumeration of all monotonic
paths, the tie rule, the beta-binomial prior, and the C ABI and size helper of include/fs2hip_align.h."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import _align as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_align.h")
U = 2.0 ** -52


@pytest.fixture(scope="module")
def fx():
    return A.load_golden()


def test_fixture_is_the_case_table(fx):
    assert [tuple(c) for c in fx["cases"]] == list(A.CASES) and float(fx["blank"]) == A.BLANK
    assert os.path.getsize(A.GOLDEN) < 1 << 20
    _, mats = A.batch_logp(np.float64)
    for b, ((T, L), m) in enumerate(zip(A.CASES, mats)):
        assert fx[f"x{b}"].shape == (T, L) and fx[f"x{b}"].dtype == np.float64
        np.testing.assert_array_equal(fx[f"x{b}"], m)
        for tag in ("", "32_"):
            d = fx[f"dur{tag}{b}"]
            assert d.dtype == np.int64 and d.shape == (L,) and d.min() >= 1 and d.sum() == T
            np.testing.assert_array_equal(np.repeat(np.arange(L), d), fx[f"path{tag}{b}"])
    assert max(T for T, _ in A.CASES) <= A.T_MAX and max(L for _, L in A.CASES) <= A.L_MAX
    assert np.isfinite(fx["nll"]).all() and np.isfinite(fx["score"]).all()


def test_restatement_agrees_with_torch_ctc(fx):
    """nll and gradient of the restatement against torch's CPU float64 ctc_loss and autograd, under
    the bounds the GPU tests hold the kernels to."""
    for tag, cast in (("", np.float64), ("32", np.float32)):
        sep = "_" if tag else ""
        for b, (T, L) in enumerate(A.CASES):
            nll, grad, _ = A.forward_sum_ref(fx[f"x{b}"].astype(cast))
            want = fx[f"nll{tag}"][b]
            assert abs(nll - want) <= 8 * T * U * abs(want), (tag, b, nll, want)
            err = np.abs(grad - fx[f"grad{tag}{sep}{b}"]).max()
            assert err <= 16 * T * max(want, 1.0) * U, (tag, b, err)


def test_forward_sum_ref_infeasible_and_occupancy():
    nll, grad, _ = A.forward_sum_ref(A.make_logp(4, 5, 1))
    assert nll == np.inf and grad.shape == (4, 5) and not grad.any()
    # softmax - occupancy: over the L + 1 classes both sum to 1 per frame, so the L label columns sum to
    # minus the blank's entry, which lies in [-1, 1]
    x = A.make_logp(9, 4, 2)
    _, grad, _ = A.forward_sum_ref(x)
    assert (np.abs(grad) <= 1.0).all() and (np.abs(grad.sum(axis=1)) <= 1.0).all()


def test_mas_ref_is_the_best_monotonic_path():
    rng = np.random.default_rng(5)
    for T in range(1, 8):
        for L in range(1, min(T, 4) + 1):
            for trial in range(3):
                x = A.make_logp(T, L, 1000 + 100 * T + 10 * L + trial) if trial else rng.standard_normal((T, L))
                dur, score, path = A.mas_ref(x)
                best, arg = A.mas_brute(x)
                assert score == best and tuple(dur) in arg, (T, L, trial)
                assert dur.min() >= 1 and dur.sum() == T
                np.testing.assert_array_equal(np.repeat(np.arange(L), dur), path)
    assert A.mas_ref(np.zeros((2, 3)))[0] is None and A.mas_ref(np.zeros((2, 3)))[1] == -np.inf


def test_tie_rule_and_hand_built_path():
    dur, score, _ = A.mas_ref(np.zeros((5, 3)))
    assert list(dur) == [3, 1, 1] and score == 0.0  # a tie takes the diagonal; the other rule gives [1, 1, 3]
    want = [2, 1, 4, 1, 3]
    dur, score, _ = A.mas_ref(A.path_matrix(want, 11, 5))
    assert list(dur) == want and score == 0.0


def test_beta_binomial_prior_rows_sum_to_one():
    from fs2amd.align import beta_binomial_prior

    for L, T, s in ((1, 1, 1.0), (1, 7, 1.0), (5, 5, 1.0), (9, 40, 1.0), (17, 33, 0.5), (70, 136, 2.0)):
        p = beta_binomial_prior(L, T, s)
        assert p.shape == (T, L) and p.dtype == np.float64 and (p >= 0).all()
        np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    p = beta_binomial_prior(9, 40)
    assert p[0].argmax() == 0 and p[-1].argmax() == 8  # the diagonal: first frame first phoneme, last frame last
    assert (np.diff(p.argmax(axis=1)) >= 0).all()
    with pytest.raises(ValueError):
        beta_binomial_prior(0, 5)


def test_align_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_ALIGN) == ["fs2_forward_sum", "fs2_forward_sum_bwd",
                                                         "fs2_forward_sum_lds_bytes", "fs2_mas", "fs2_mas_lds_bytes",
                                                         "fs2_mas_ws_bytes"], declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO)
              | set(_lib.SIGNATURES_AUDIO_INV) | set(_lib.SIGNATURES_PREP) | set(_lib.SIGNATURES_F0)
              | set(_lib.SIGNATURES_RESAMPLE))
    assert not set(declared) & others
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_ALIGN[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_align.h" in _lib.EXTRA_HEADERS
    text = open(HEADER).read()
    for name, val in (("FS2_MAS_LDS_BYTES", _lib.MAS_LDS_BYTES), ("FS2_MAS_LDS_SMALL", _lib.MAS_LDS_SMALL),
                      ("FS2_FORWARD_SUM_LDS_BYTES", _lib.FORWARD_SUM_LDS_BYTES), ("FS2_MAS_AUTO", _lib.MAS_AUTO),
                      ("FS2_MAS_LDS", _lib.MAS_LDS), ("FS2_MAS_GLOBAL", _lib.MAS_GLOBAL)):
        assert re.search(rf"#define {name} {val}\s", text), name
    sizes = open(os.path.join(REPO, "expressive-fastspeech2-mandarin_amd", "csrc", "align_sizes.h")).read()
    assert re.search(r"#define FS2_AL_SIZE_CAP \(1 << 24\)", sizes) and _lib.ALIGN_SIZE_CAP == 1 << 24


def test_size_mirror_agrees_with_the_library():
    from fs2amd import _lib

    lib = _lib.load()
    big = (1 << 31) - 1
    sizes = (-1, 0, 1, 2, 63, 64, 65, 70, 136, 150, 860, 1000, 1279, 1280, 1281, 10238, 10239, 10240, 1 << 24,
             (1 << 24) + 1, big)
    for T in sizes:
        for Lx in sizes:
            for in_lds in (0, 1):
                assert lib.fs2_mas_lds_bytes(T, Lx, in_lds) == _lib.mas_lds_bytes(T, Lx, bool(in_lds)), (T, Lx, in_lds)
            assert lib.fs2_forward_sum_lds_bytes(T, Lx) == _lib.forward_sum_lds_bytes(T, Lx), (T, Lx)
            for B in (0, 1, 64, big):
                assert lib.fs2_mas_ws_bytes(B, T, Lx) == _lib.mas_ws_bytes(B, T, Lx), (B, T, Lx)
    # the sizes the documents quote
    assert _lib.mas_lds_bytes(860, 150) == 8 * (2 * 151 + 860 * 3) == 23056 <= _lib.MAS_LDS_SMALL
    assert _lib.mas_lds_bytes(1000, 1000) == 8 * (2 * 1001 + 1000 * 16) == 144016 <= _lib.MAS_LDS_BYTES
    assert _lib.mas_form(1000, 1000) == (_lib.FS2_OK, _lib.MAS_LDS)
    assert _lib.mas_form(1281, 1000) == (_lib.FS2_OK, _lib.MAS_GLOBAL)  # the first T past the LDS at L = 1000
    assert _lib.mas_form(1281, 1000, _lib.MAS_LDS) == (_lib.FS2_EUNSUPPORTED, None)
    assert _lib.mas_form(5, 10239) == (_lib.FS2_OK, _lib.MAS_GLOBAL) and _lib.mas_form(5, 10240)[0] == _lib.FS2_EUNSUPPORTED
    assert _lib.forward_sum_lds_bytes(1000, 1000) == 48080 <= _lib.FORWARD_SUM_LDS_BYTES


def test_size_mirror_agrees_with_the_standalone_check():
    """tools/align_sizes_check.py: the stand-alone host program over csrc/align_sizes.h prints what the
    Python mirror gives at every boundary size. The tool's own run builds it with ASan and UBSan (DESIGN
    9.5 records that run); here the same program is built plainly, so that the comparison does not
    depend on a sanitizer runtime where the suite runs."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("align_sizes_check", os.path.join(REPO, "tools", "align_sizes_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cxx = shutil.which("g++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler build() uses otherwise
    assert mod.check(cxx, sanitize=False) > 5000


def test_align_entries_reject_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    P_ = 4096  # a non-NULL pointer that is never dereferenced: every call below returns before a launch
    EINVAL, EUNSUP = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    #       logp dtype        bs        rs  mel tex B  T    L   bitmap ws  ws_bytes dur sco path stream
    good = [P_, _lib.FS2_F32, 136 * 70, 70, P_, P_, 8, 136, 70, 0, None, 0, P_, P_, P_, None]

    def call(fn, base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)

    mas = lib.fs2_mas
    assert call(mas, good, a0=None) == EINVAL and call(mas, good, a12=None) == EINVAL and call(mas, good, a13=None) == EINVAL
    for k in (6, 7, 8):
        assert call(mas, good, **{f"a{k}": 0}) == EINVAL and call(mas, good, **{f"a{k}": -2}) == EINVAL, k
    assert call(mas, good, a3=69) == EINVAL and call(mas, good, a2=135 * 70 + 69) == EINVAL  # overlapping rows
    assert call(mas, good, a9=3) == EINVAL and call(mas, good, a9=-1) == EINVAL
    assert call(mas, good, a9=_lib.MAS_GLOBAL) == EINVAL  # no workspace
    assert call(mas, good, a9=_lib.MAS_GLOBAL, a10=P_, a11=_lib.mas_ws_bytes(8, 136, 70) - 1) == EINVAL
    for bad in (_lib.FS2_BF16, _lib.FS2_FP8, _lib.FS2_I16, 9):
        assert call(mas, good, a1=bad) == EUNSUP
    assert call(mas, good, a7=1281, a8=1000, a2=1281 * 1000, a3=1000, a9=_lib.MAS_LDS) == EUNSUP
    assert call(mas, good, a7=1281, a8=1000, a2=1281 * 1000, a3=1000) == EINVAL  # auto -> global: no workspace
    assert call(mas, good, a8=10240, a3=10240, a2=136 * 10240, a10=P_, a11=1 << 40) == EUNSUP  # the rows alone
    #      logp dtype        bs        rs  mel tex B  T    L   blank alpha nll loss stream
    fwd = [P_, _lib.FS2_F64, 136 * 70, 70, P_, P_, 8, 136, 70, -1.0, P_, P_, P_, None]
    fs = lib.fs2_forward_sum
    for k in (0, 10, 11, 12):
        assert call(fs, fwd, **{f"a{k}": None}) == EINVAL, k
    assert call(fs, fwd, a9=float("nan")) == EINVAL and call(fs, fwd, a9=float("-inf")) == EINVAL
    assert call(fs, fwd, a1=_lib.FS2_BF16) == EUNSUP
    assert call(fs, fwd, a7=4096, a8=2048, a2=4096 * 2048, a3=2048) == EUNSUP
    #      logp dtype        bs        rs  mel tex B  T    L   blank alpha nll gout grad stream
    bwd = [P_, _lib.FS2_F64, 136 * 70, 70, P_, P_, 8, 136, 70, -1.0, P_, P_, P_, P_, None]
    fb = lib.fs2_forward_sum_bwd
    for k in (0, 10, 11, 12, 13):
        assert call(fb, bwd, **{f"a{k}": None}) == EINVAL, k
    assert call(fb, bwd, a8=0) == EINVAL and call(fb, bwd, a1=_lib.FS2_I16) == EUNSUP
    assert call(fb, bwd, a7=4096, a8=2048, a2=4096 * 2048, a3=2048) == EUNSUP


def test_align_api_is_exported_and_refuses_cpu_tensors():
    import fs2amd
    import fs2amd.align
    import fs2amd.library as lib
    from fs2amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name in ("ForwardSumLoss", "AlignmentEncoder", "mas_durations", "fit_aligner"):
        assert hasattr(fs2amd, name) and name in fs2amd.__all__
    x = torch.zeros(2, 6, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mas(x, [6, 6], [3, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.forward_sum(x, [6, 6], [3, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.ForwardSumLoss()(x, [6, 6], [3, 3])
    assert lib.OPS_ALIGN == ("mas", "forward_sum", "forward_sum_bwd") and all(hasattr(torch.ops.fs2, n) for n in lib.OPS_ALIGN)
    assert not set(lib.OPS_ALIGN) & (set(lib.OPS) | set(lib.OPS_PREP) | set(lib.OPS_F0) | set(lib.OPS_RESAMPLE))
    for op in lib.OPS_ALIGN:
        assert f"fs2::{op}" in lib.__doc__
    with FakeTensorMode():
        logp = torch.empty(3, 50, 7, device="cuda")
        dur, score, path = torch.ops.fs2.mas(logp, None, None)
        assert dur.shape == (3, 7) and dur.dtype == torch.int64 and score.shape == (3,) and path.shape == (3, 50)
        loss, nll, alpha = torch.ops.fs2.forward_sum(logp, None, None, -1.0)
        assert loss.shape == () and loss.dtype == torch.float64 and nll.shape == (3,) and alpha.shape == (3, 50, 15)
        g = torch.ops.fs2.forward_sum_bwd(logp, None, None, alpha, nll, loss, -1.0)
        assert g.shape == logp.shape and g.dtype == logp.dtype


def test_alignment_encoder_on_the_cpu_masks_and_normalises():
    """The encoder is plain torch: its output is a log-probability over each utterance's own phonemes
    (before the prior), -inf beyond them, and the distance it scores is the squared difference."""
    from fs2amd.align import AlignmentEncoder

    torch.manual_seed(0)
    enc = AlignmentEncoder(12, n_mel=8, d_text=16, d_att=6, temperature=0.05, prior=False)
    ids = torch.randint(0, 12, (2, 5))
    mels = torch.randn(2, 9, 8)
    out = enc(ids, [5, 3], mels, [9, 7])
    assert out.shape == (2, 9, 5) and out.dtype == torch.float32
    assert torch.isinf(out[1, :, 3:]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[1, :, :3]).all()
    np.testing.assert_allclose(out[1, :7, :3].exp().sum(1).detach().numpy(), 1.0, atol=1e-5)
    k = enc.key_proj(enc.embedding(ids).transpose(1, 2))
    q = enc.query_proj(mels.transpose(1, 2)).transpose(1, 2)
    d = ((q[0, :, None, :] - k[0].t()[None, :, :]) ** 2).sum(-1)
    np.testing.assert_allclose(out[0].detach().numpy(), torch.log_softmax(-0.05 * d, dim=1).detach().numpy(), atol=1e-4)
    with_prior = AlignmentEncoder(12, n_mel=8, d_text=16, d_att=6, prior=True)
    lp = with_prior.log_prior([5, 3], [9, 7], 9, 5, "cpu")
    assert lp.shape == (2, 9, 5) and float(lp[1, 7:].abs().max()) == 0.0
