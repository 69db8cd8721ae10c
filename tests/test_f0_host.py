"""F0 estimation, host side (no GPU): the numpy restatement of tests/_f0.py against the true F0 of the
synthetic waveforms in tests/golden/f0_a.npz, its order independence on int16 input, the absence of
fragile frames in the general float32 case, and the C ABI of include/fs2hip_f0.h."""
import os
import re

import numpy as np
import pytest
import torch

import _f0 as Y

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_f0.h")
STEADY = ("tone75", "tone100", "tone163.7", "tone220", "tone440", "tone780")


@pytest.fixture(scope="module")
def fx():
    return Y.load_fixture()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def interior(fx, name, margin=4):
    b = list(fx["names16"]).index(name)
    F = Y.n_frames(int(fx["lens16"][b]), Y.HOP)
    sl = slice(margin, F - margin)
    return fx["f0_16"][b, sl], fx["truth16"][b, sl]


def test_fixture_has_the_cases_the_kernel_can_get_wrong(fx):
    lens = set(int(n) for n in fx["lens16"])
    assert {0, 1, 255, 256, 257, 512, 1334, 1335, 1336} <= lens and max(lens) > 9000
    tau_min, tau_max = Y.lags()
    assert (tau_min, tau_max) == (27, 311) and 1335 == Y.WIN + tau_max
    assert fx["tau_16"].max() == tau_max - 1  # a lag on the last admissible entry
    names = list(fx["names16"])
    for b in (names.index("splice_a"), names.index("splice_b")):  # voicing switches inside a frame group
        F = Y.n_frames(int(fx["lens16"][b]), Y.HOP)
        v = fx["f0_16"][b, :F] > 0
        groups = [v[g:g + 8] for g in range(0, F, 8)]
        assert any(g.any() and not g.all() for g in groups)
    assert fx["wav32"].dtype == np.float32 and fx["wav16"].dtype == np.int16
    twin = fx["wav16"][int(fx["twin16"]), :fx["lens32"][0]]
    assert (fx["wav32"][0, :fx["lens32"][0]].astype(np.float64) * 32768.0 == twin).all()
    g = fx["wav32"][1, :fx["lens32"][1]].astype(np.float64) * 32768.0
    assert (g != np.round(g)).mean() > 0.9  # the general case is not dyadic
    assert os.path.getsize(os.path.join(Y.GOLDEN, "f0_a.npz")) < 400 * 1024


def test_stored_contours_are_the_restatements(fx):
    for key, lens_key, hop, W in (("16", "lens16", Y.HOP, Y.WIN), ("200", "lens200", 200, 800),
                                  ("32", "lens32", Y.HOP, Y.WIN)):
        for b, w in enumerate(Y.ragged(fx, "wav" + key, lens_key)):
            f0, tau, _ = Y.contour(w, hop=hop, W=W)
            F = Y.n_frames(len(w), hop)
            assert len(f0) == F
            np.testing.assert_array_equal(bits(f0), bits(fx["f0_" + key][b, :F]))
            np.testing.assert_array_equal(tau, fx["tau_" + key][b, :F])
            assert (fx["f0_" + key][b, F:] == 0).all() and (fx["tau_" + key][b, F:] == 0).all()
            assert ((f0 == 0) == (tau == 0)).all() and ((f0 == 0) | ((f0 >= Y.F0_FLOOR) & (f0 <= Y.F0_CEIL))).all()
    np.testing.assert_array_equal(bits(fx["f0_32"][0]), bits(fx["f0_16"][int(fx["twin16"]), :fx["f0_32"].shape[1]]))


def test_restatement_against_ground_truth(fx):
    worst = {}
    for name in STEADY:
        f0, truth = interior(fx, name)
        assert len(f0) >= 4 and (f0 > 0).all(), name
        worst[name] = float(np.abs(f0 / truth - 1).max())
    f0, truth = interior(fx, "glide120_200")
    assert (f0 > 0).all()
    glide = float(np.abs(f0 / truth - 1).max())
    f0, truth = interior(fx, "missing_fundamental")
    assert (f0 > 0).all()
    missing = float(np.abs(f0 / 150.0 - 1).max())
    print("relative error of the restatement:", worst, "glide", glide, "missing fundamental", missing)
    assert max(worst.values()) <= 2e-3 and glide <= 1.5e-2 and missing <= 2e-3
    names = list(fx["names16"])
    for name in ("noise", "silence", "silence_0"):
        assert not (fx["f0_16"][names.index(name)] > 0).any(), name
    # above the range: unvoiced, or the sub-octave the restatement finds
    f860 = fx["f0_16"][names.index("tone860")]
    assert ((f860 == 0) | (np.abs(f860 / 430.0 - 1) < 2e-3)).all()


def test_int16_table_does_not_depend_on_the_summation_order(fx):
    for key, lens_key, hop, W in (("16", "lens16", Y.HOP, Y.WIN), ("200", "lens200", 200, 800)):
        for w in Y.ragged(fx, "wav" + key, lens_key):
            d0, dp0 = Y.table(w, hop, W, order="forward")
            assert d0.max(initial=0) * Y.lags()[1] < 2.0 ** 53
            for order in ("backward", "blocks"):
                d, dp = Y.table(w, hop, W, order=order)
                np.testing.assert_array_equal(bits(d), bits(d0))
                np.testing.assert_array_equal(bits(dp), bits(dp0))
    w = fx["wav32"][0, :fx["lens32"][0]]  # samples k * 2^-15: exact as well
    np.testing.assert_array_equal(bits(Y.table(w, order="blocks")[1]), bits(Y.table(w, order="forward")[1]))


def test_general_float32_case_has_no_fragile_frame(fx):
    w = fx["wav32"][1, :fx["lens32"][1]]
    dp = Y.table(w)[1]
    assert Y.fragile(dp) == []
    # and the orders agree within the header's bound, so the picks agree
    tau_max = Y.lags()[1]
    bound = Y.dp_ulps(Y.WIN, np.arange(tau_max + 1)) * Y.U
    for order in ("backward", "blocks"):
        other = Y.table(w, order=order)[1]
        assert (np.abs(other - dp) <= bound[None, :] * np.abs(dp)).all()
        np.testing.assert_array_equal(Y.contour_of_table(other)[1], fx["tau_32"][1, :len(dp)])
    assert (fx["f0_32"][1, 4:len(dp) - 4] > 0).all()


def test_f0_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_F0) == ["fs2_f0_lds_bytes", "fs2_f0_yin"], declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO)
              | set(_lib.SIGNATURES_AUDIO_INV) | set(_lib.SIGNATURES_PREP))
    assert not set(declared) & others
    assert not set(declared) & set(_lib.header_symbols(_lib.HEADER_PREP))
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_F0[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_f0.h" in _lib.EXTRA_HEADERS
    text = open(HEADER).read()
    for name, val in (("FS2_F0_GROUP", _lib.F0_GROUP), ("FS2_F0_LDS_BYTES", _lib.F0_LDS_BYTES)):
        assert re.search(rf"#define {name} {val}\s", text), name
    m = re.search(r"#define FS2_F0_DP_ULPS\(W, tau\) \((.*)\)\n", text)
    expr = m.group(1).replace("(W)", "W").replace("(tau)", "tau")
    for W, tau in ((1024, 311), (800, 27), (1, 2)):
        assert eval(expr, {"W": W, "tau": tau}) == _lib.f0_dp_ulps(W, tau) == Y.dp_ulps(W, tau)
    assert lib.fs2_f0_lds_bytes(256, 1024, 311) == 55704 and "tau_max 311: 55704" in text


def lds_formula(hop, W, tau_max, G=8):
    """The formula the header states beside FS2_F0_LDS_BYTES."""
    tau_pad = (tau_max + 7) // 8 * 8
    q, r = divmod(W, hop)
    segs = (G + q - 1 if q else 0) + (G if r else 0)
    span = (G - 1) * hop + W + tau_pad
    return 8 * (max(span + span // 8 + 1, G * (tau_pad + 1)) + segs * (tau_pad + 1))


def test_f0_lds_bytes_is_the_headers_formula():
    from fs2amd import _lib

    size = _lib.load().fs2_f0_lds_bytes
    sizes = (1, 2, 7, 8, 9, 199, 200, 255, 256, 257, 311, 312, 313, 800, 1024, 1025, 4096, 1 << 24)
    for hop in sizes:
        for W in sizes:
            for tau_max in sizes:
                assert size(hop, W, tau_max) == lds_formula(hop, W, tau_max, _lib.F0_GROUP), (hop, W, tau_max)
    for bad in ((0, 1024, 311), (256, 0, 311), (256, 1024, 0), (-1, 1024, 311)):
        assert size(*bad) == 0
    for huge in (((1 << 24) + 1, 1024, 311), (256, (1 << 31) - 1, 311), (256, 1024, (1 << 31) - 1), ((1 << 31) - 1,) * 3):
        assert size(*huge) == (1 << 63) - 1  # saturates: nothing overflows
    # the largest W that fits at hop 256 and lags up to 311, and the first that does not
    fit = max(W for W in range(1024, 4096) if lds_formula(256, W, 311) <= _lib.F0_LDS_BYTES)
    assert size(256, fit, 311) <= _lib.F0_LDS_BYTES < min(size(256, fit + 1, 311), size(256, fit + 256, 311))


def test_f0_entry_rejects_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    P_ = 4096  # a non-NULL pointer that is never dereferenced: every call below returns before a launch
    EINVAL, EUNSUP = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    I16, F32 = _lib.FS2_I16, _lib.FS2_F32
    yin = lib.fs2_f0_yin
    #       wav dtype stride lens B n_max sr      hop  W     tmin tmax thr  floor ceil   f0  tau cmnd stream
    good = [P_, I16, 4000, P_, 2, 4000, 22050.0, 256, 1024, 27, 311, 0.1, 71.0, 800.0, P_, P_, P_, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return yin(*a)

    assert call(a0=None) == EINVAL and call(a14=None) == EINVAL  # wav, f0
    for k in (4, 5, 7, 8):  # B, n_max, hop, W
        assert call(**{f"a{k}": 0}) == EINVAL and call(**{f"a{k}": -3}) == EINVAL, k
    assert call(a2=3999) == EINVAL  # stride below the width
    assert call(a9=1) == EINVAL and call(a9=0) == EINVAL  # tau_min < 2
    assert call(a9=311) == EINVAL and call(a9=400) == EINVAL  # tau_min >= tau_max
    for bad in (_lib.FS2_BF16, _lib.FS2_FP8, _lib.FS2_F64, 9):
        assert call(a1=bad) == EUNSUP
    assert call(a4=65536) == EUNSUP
    # the LDS limit, on each of its three sides; the largest sizes that still fit are accepted by the formula
    assert lib.fs2_f0_lds_bytes(256, 1024, 311) <= _lib.F0_LDS_BYTES
    for hop, W, tau_max in ((256, 2048, 311), (256, 1024, 600), (1024, 1024, 311), (1, 1024, 311), (256, 1 << 30, 311),
                            (256, 1024, 1 << 30), (1 << 30, 1024, 311), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        assert lib.fs2_f0_lds_bytes(hop, W, tau_max) > _lib.F0_LDS_BYTES
        assert call(a7=hop, a8=W, a10=tau_max) == EUNSUP, (hop, W, tau_max)


def test_f0_api_is_exported_and_refuses_cpu_tensors():
    import fs2amd
    import fs2amd.library as lib
    from fs2amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert hasattr(fs2amd, "f0_contour") and "f0_contour" in fs2amd.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.f0_yin(torch.zeros(2, 4000, dtype=torch.int16), sampling_rate=22050, hop_length=256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.f0_contour([np.zeros(100, dtype=np.int16)], sampling_rate=22050, hop_length=256, device="cpu")
    assert ops.f0_lags(22050, 71.0, 800.0) == Y.lags() == (27, 311)
    assert lib.OPS_F0 == ("f0_yin",) and all(hasattr(torch.ops.fs2, n) for n in lib.OPS_F0)
    assert not set(lib.OPS_F0) & (set(lib.OPS) | set(lib.OPS_PREP))
    with FakeTensorMode():
        wav = torch.empty(3, 5000, device="cuda", dtype=torch.int16)
        f0, tau, cmnd = torch.ops.fs2.f0_yin(wav, None, 22050.0, 256, 1024, 71.0, 800.0, 0.1)
        assert f0.shape == tau.shape == (3, 20) and cmnd.shape == (3, 20, 312)
        assert f0.dtype == cmnd.dtype == torch.float64 and tau.dtype == torch.int32
