"""F0 tracking, host side (no GPU): the numpy restatement of tests/_f0_track.py against the true F0 of
the synthetic waveforms in tests/golden/f0_track_a.npz and against plain YIN on the cases built to
defeat it, the conditions the fixture has to meet (no ties that count, no fragile comparison), the
tie order on a hand-built table, the host tables of fs2amd.f0, and the C ABI of
include/fs2hip_f0_track.h."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import _f0 as Y
import _f0_track as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_f0_track.h")


@pytest.fixture(scope="module")
def fx():
    return T.load_fixture()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_fixture_has_the_cases_the_issue_lists(fx):
    lens = set(int(n) for n in fx["lens16"])
    assert {0, 1, 255, 256, 257, 1335} <= lens and 3000 in lens and 9000 <= max(lens) <= 9216
    names = set(fx["names16"])
    assert set(T.STEADY) | {"glide120_200", "missing_fundamental", "noise", "silence", "splice", "trap", "weak"} <= names
    assert fx["wav16"].dtype == np.int16 and fx["wav200"].dtype == np.int16 and fx["wav32"].dtype == np.float32
    assert len(fx["lens200"]) == 2
    twin = fx["wav16"][int(fx["twin16"]), :fx["lens32"][0]]
    assert (fx["wav32"][0, :fx["lens32"][0]].astype(np.float64) * 32768.0 == twin).all()
    g = fx["wav32"][1, :fx["lens32"][1]].astype(np.float64) * 32768.0
    assert (g != np.round(g)).mean() > 0.9  # the general case is not dyadic
    assert os.path.getsize(os.path.join(T.GOLDEN, "f0_track_a.npz")) < 400 * 1024
    for name in T.STEADY + ("glide120_200", "missing_fundamental", "trap", "weak"):  # interior: three quarters at least
        F = Y.n_frames(int(fx["lens16"][list(fx["names16"]).index(name)]), Y.HOP)
        assert 2 * T.MARGIN <= F // 4, name


def test_stored_paths_are_the_restatements(fx):
    tb = T.tables()
    assert (tb.N, tb.tau_min, tb.tau_max) == (210, 27, 311)
    for key, hop, W in (("16", Y.HOP, Y.WIN), ("200", 200, 800), ("32", Y.HOP, Y.WIN)):
        for b, w in enumerate(Y.ragged(fx, "wav" + key, "lens" + key)):
            f0, state, score, _, _, _ = T.track(w, tb, hop, W)
            F = Y.n_frames(len(w), hop)
            assert len(f0) == F
            np.testing.assert_array_equal(bits(f0), bits(fx["f0_" + key][b, :F]))
            np.testing.assert_array_equal(state, fx["state_" + key][b, :F])
            assert bits(score) == bits(fx["score_" + key][b])
            assert (fx["f0_" + key][b, F:] == 0).all() and (fx["state_" + key][b, F:] == -1).all()
            assert ((f0 == 0) == (state == -1)).all() and ((f0 == 0) | ((f0 >= Y.F0_FLOOR) & (f0 <= Y.F0_CEIL))).all()
    F32 = fx["f0_32"].shape[1]
    twin = int(fx["twin16"])
    np.testing.assert_array_equal(bits(fx["f0_32"][0]), bits(fx["f0_16"][twin, :F32]))
    assert bits(fx["score_32"][0]) == bits(fx["score_16"][twin])


def test_fixture_meets_its_conditions(fx, capsys):
    """Interior voiced frames of the tones, the glide and the missing fundamental within 2e-3, 1.5e-2
    and 2e-3 of the truth (the bounds tests/test_f0_host.py sets for the same refinement); no voiced
    frame in noise and silence; plain YIN misses interior frames of the trap and the weak trough and
    the path none; no tie that counts on an int16 case; no fragile comparison in the general float32
    case. T.fixture_faults prints the figures."""
    with capsys.disabled():
        faults = T.fixture_faults(fx, verbose=True)
    assert faults == []


def test_trap_and_weak_trough_defeat_plain_yin_only(fx):
    tb = T.tables()
    names = list(fx["names16"])
    for name, kind in (("trap", "octave"), ("weak", "dropped")):
        b = names.index(name)
        n = int(fx["lens16"][b])
        F = Y.n_frames(n, Y.HOP)
        sl = slice(T.MARGIN, F - T.MARGIN)
        truth = fx["truth16"][b, :F][sl]
        yin = Y.contour(fx["wav16"][b, :n])[0][sl]
        assert T.wrong(yin, truth).any()
        if kind == "octave":
            assert (np.abs(yin / truth - 0.5) < 0.03).any()  # the lower octave
        else:
            assert (yin == 0).any() and (yin > 0).any()  # it flickers
        assert not T.wrong(fx["f0_16"][b, :F][sl], truth).any()


def viterbi_loops(obs_v, obs_u, tb):
    """The recursion of the header a second time, state by state and predecessor by predecessor in
    the stated order: what the dense numpy of tests/_f0_track.py has to agree with where sums tie."""
    F, N, K = len(obs_u), tb.N, tb.K
    delta = [list(obs_v[0] + tb.LINIT) + [obs_u[0] + tb.LINIT] * N]
    back = [None]
    for k in range(1, F):
        row, brow = [], []
        for s in range(2 * N):
            voiced, n = s < N, s % N
            best, arg = -np.inf, None
            for j in range(max(n - K, 0), min(n + K, N - 1) + 1):
                for same in (True, False):
                    sp = j + (0 if voiced == same else N)
                    v = delta[-1][sp] + (tb.TS if same else tb.TX)[abs(n - j)]
                    if v > best:
                        best, arg = v, sp
            row.append((obs_v[k][n] if voiced else obs_u[k]) + best)
            brow.append(arg)
        delta.append(row)
        back.append(brow)
    s = max(range(2 * N), key=lambda i: (delta[-1][i], -i))
    score, path = delta[-1][s], [s]
    for k in range(F - 1, 0, -1):
        s = back[k][s]
        path.append(s)
    return np.array(path[::-1]), float(score)


def test_tie_order_on_a_hand_built_table():
    tb, cmnd = T.tie_case()
    assert (tb.N, tb.K, tb.tau_min, tb.tau_max) == (28, 3, 4, 20) and cmnd.shape == (5, 21)
    # troughs at lags 8, 10, 13 with equal neighbours: p = t exactly, bins 15, 12, 7, every mass 0
    cands, g = T.frame_candidates(cmnd[0], tb)
    assert [(c[0], c[1], c[2], c[3]) for c in cands] == [(15, 0.0, 125.0, 8), (12, 0.0, 100.0, 10), (7, 0.0, 1000.0 / 13, 13)]
    assert g == 10  # the smallest dp is 0.10: a = 11
    obs_v, obs_u, _ = T.observations(cmnd, tb)
    f0, state, score, path, ties, final_tie = T.track_table(cmnd, tb)
    lp, ls = viterbi_loops(obs_v, obs_u, tb)
    np.testing.assert_array_equal(path, lp)
    assert score == ls == -1.0  # log_init and five masses of 0
    # Bins 12 and 15 are within a step of 3 and both hold a candidate in frames 0, 1, 2 and 4: every
    # chain over them sums to -1. The lower bin is the first predecessor and the lowest final state.
    assert ties[1:4].all() and final_tie
    np.testing.assert_array_equal(state, np.full(5, 12, dtype=np.int32))
    np.testing.assert_array_equal(f0, np.full(5, 100.0))


def test_dense_viterbi_agrees_with_the_loops_on_a_fixture_case(fx):
    tb = T.tables()
    b = list(fx["names16"]).index("tone220_1335")
    dp = Y.table(fx["wav16"][b, :1335], Y.HOP, Y.WIN, tb.tau_max)[1]
    obs_v, obs_u, _ = T.observations(dp, tb)
    path, score, _, _ = T.viterbi(obs_v, obs_u, tb)
    lp, ls = viterbi_loops(obs_v, obs_u, tb)
    np.testing.assert_array_equal(path, lp)
    assert bits(score) == bits(ls)


def test_package_tables_are_the_restatements():
    from fs2amd.f0 import F0TrackTables, f0_track_tables

    for kw in (dict(), T.TIE_PARAMS):
        tb = T.tables(**kw)
        pk = f0_track_tables(tb.sr, tb.f0_floor, tb.f0_ceil, tb.R, tb.K, 0.01)
        assert isinstance(pk, F0TrackTables) and pk is f0_track_tables(tb.sr, tb.f0_floor, tb.f0_ceil, tb.R, tb.K, 0.01)
        assert (pk.n_bins, pk.max_step) == (tb.N, tb.K)
        for mine, theirs in ((tb.S, pk.thr), (tb.LM0, pk.lm0), (tb.LM1, pk.lm1), (tb.LU, pk.lu), (tb.E, pk.edges),
                             (tb.TS, pk.trans_same), (tb.TX, pk.trans_switch), (tb.FLOOR, pk.log_floor),
                             (tb.LINIT, pk.log_init)):
            np.testing.assert_array_equal(bits(mine), bits(theirs))
    tb = T.tables()
    # a sample of entries against the platform's own logarithm: correctly rounded values lie within an ulp of it
    for u, v in ((0, 100), (5, 15), (10, 100), (60, 99)):
        assert abs(tb.LM0[u, v] - max(np.log(float(tb.C[v] - tb.C[u])), tb.FLOOR)) <= 4e-15 * abs(tb.LM0[u, v]) + 1e-300
    assert tb.LM0[0, 100] == 0.0 and tb.LM1[0, 0] == -np.inf and tb.LM0[7, 7] == -np.inf
    assert abs(tb.LU[101] - np.log(1 / 210)) < 1e-14
    assert len(tb.E) == 211 and tb.E[0] >= 22050 / 71.0 * (1 - 1e-15) and tb.E[210] <= 22050 / 800.0
    assert tb.E[209] > 22050 / 800.0  # N is the smallest count that reaches f0_ceil
    with pytest.raises(ValueError):
        F0TrackTables(22050, 800.0, 71.0)


def test_f0_track_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_F0_TRACK) == ["fs2_f0_track", "fs2_f0_track_lds_bytes",
                                                            "fs2_f0_track_workspace_bytes"], declared
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO) | set(_lib.SIGNATURES_F0)
              | set(_lib.SIGNATURES_AUDIO_INV) | set(_lib.SIGNATURES_PREP) | set(_lib.SIGNATURES_EVAL))
    assert not set(declared) & others
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_F0_TRACK[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_f0_track.h" in _lib.EXTRA_HEADERS and _lib.HEADER_F0_TRACK == HEADER
    text = open(HEADER).read()
    for name, val in (("FS2_F0_TRACK_THR", _lib.F0_TRACK_THR), ("FS2_F0_TRACK_CAP_MAX", _lib.F0_TRACK_CAP_MAX),
                      ("FS2_F0_TRACK_BINS_MAX", _lib.F0_TRACK_BINS_MAX), ("FS2_F0_TRACK_STEP_MAX", _lib.F0_TRACK_STEP_MAX),
                      ("FS2_F0_TRACK_TB", _lib.F0_TRACK_TB), ("FS2_F0_TRACK_LDS_BYTES", _lib.F0_TRACK_LDS_BYTES)):
        assert re.search(rf"#define {name} {val}\s", text), name
    assert T.N_THR == _lib.F0_TRACK_THR
    import __graft_entry__ as g

    assert "f0_track.hip" in g.HIP_SOURCES


def test_sizes_are_the_headers_formula():
    from fs2amd import _lib

    lib = _lib.load()
    ws, lds = lib.fs2_f0_track_workspace_bytes, lib.fs2_f0_track_lds_bytes
    # the benchmark's batch: 8 B of head, 101 entries of 20 B and 420 predecessor bytes per frame
    assert _lib.f0_track_cap(27, 311) == 101 and _lib.f0_track_cap(4, 20) == 8 and _lib.f0_track_cap(2, 3) == 1
    assert ws(64, 860, 27, 311, 210) == 64 * 860 * (8 + 101 * 20 + 420) == _lib.f0_track_workspace_bytes(64, 860, 27, 311, 210)
    assert lds(210, 12) == 8 * (4 * 234 + 420) + 64 * 420 + 8 == _lib.f0_track_lds_bytes(210, 12) <= _lib.F0_TRACK_LDS_BYTES
    assert lds(256, 63) <= _lib.F0_TRACK_LDS_BYTES  # the largest sizes the kernel takes fit
    for B in (1, 3, 65535, (1 << 31) - 1):
        for F in (1, 37, 860, (1 << 31) - 1):
            for lags in ((2, 3), (4, 20), (27, 311), (2, (1 << 31) - 1)):
                for N in (1, 28, 210, 256, (1 << 31) - 1):
                    assert ws(B, F, *lags, N) == _lib.f0_track_workspace_bytes(B, F, *lags, N), (B, F, lags, N)
    assert ws((1 << 31) - 1, (1 << 31) - 1, 2, (1 << 31) - 1, (1 << 31) - 1) == (1 << 63) - 1  # saturates
    for bad in ((0, 5, 27, 311, 210), (5, 0, 27, 311, 210), (5, 5, 1, 311, 210), (5, 5, 311, 311, 210), (5, 5, 27, 311, 0)):
        assert ws(*bad) == 0 == _lib.f0_track_workspace_bytes(*bad)
    assert lds(0, 12) == 0 and lds(210, -1) == 0 and lds((1 << 24) + 1, 12) == (1 << 63) - 1


def test_size_mirror_agrees_with_the_standalone_check():
    """tools/f0_track_sizes_check.py: the stand-alone host program over csrc/f0_track_sizes.h compares
    the header with a 128-bit restatement up to INT32_MAX and prints what the Python mirror has to give.
    The tool's own run builds it with ASan and UBSan (DESIGN 9.7 records that run); here the same
    program is built plainly, so that the comparison does not depend on a sanitizer runtime."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("f0_track_sizes_check",
                                                  os.path.join(REPO, "tools", "f0_track_sizes_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cxx = shutil.which("g++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler build() uses otherwise
    assert mod.check(cxx, sanitize=False) > 5000


def reject_cases():
    """(keyword overrides of a good call, expected status) for fs2_f0_track: every call returns before a launch."""
    from fs2amd import _lib

    EINVAL, EUNSUP = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    cases = [({k: None}, EINVAL) for k in ("cmnd", "thr", "lm0", "lm1", "lu", "edges", "ts", "tx", "ws", "f0", "state")]
    for k in ("B", "F_max", "hop", "N"):
        cases += [({k: 0}, EINVAL), ({k: -3}, EINVAL)]
    cases += [({"K": -1}, EINVAL), ({"sr": 0.0}, EINVAL), ({"sr": float("nan")}, EINVAL),
              ({"tau_min": 1}, EINVAL), ({"tau_min": 311}, EINVAL), ({"tau_min": 400}, EINVAL),
              ({"ws_bytes": 64 * 860 * (8 + 101 * 20 + 420) - 1}, EINVAL), ({"ws": 4100}, EINVAL),  # too small; misaligned
              ({"B": 65536, "ws_bytes": (1 << 62)}, EUNSUP), ({"N": 257}, EUNSUP), ({"K": 64}, EUNSUP),
              ({"N": (1 << 31) - 1}, EUNSUP), ({"K": (1 << 31) - 1}, EUNSUP),
              ({"F_max": (1 << 31) - 1, "ws_bytes": (1 << 62)}, EUNSUP)]
    return cases


def call_entry(lib, **kw):
    P_ = 4096  # a non-NULL pointer that is never dereferenced
    a = dict(cmnd=P_, lens=P_, B=64, F_max=860, hop=256, sr=22050.0, tau_min=27, tau_max=311, f0_floor=71.0, f0_ceil=800.0,
             thr=P_, lm0=P_, lm1=P_, lu=P_, edges=P_, N=210, ts=P_, tx=P_, K=12, log_floor=-27.0, log_init=-6.0, ws=P_,
             ws_bytes=64 * 860 * (8 + 101 * 20 + 420), f0=P_, state=P_, score=P_, stream=None)
    a.update(kw)
    return lib.fs2_f0_track(*a.values())


def test_f0_track_entry_rejects_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    for kw, status in reject_cases():
        assert call_entry(lib, **kw) == status, kw


def test_f0_track_api_is_exported_and_refuses_cpu_tensors():
    import inspect

    import fs2amd
    import fs2amd.library as lib
    from fs2amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.f0_track(torch.zeros(2, 5, 312, dtype=torch.float64), sampling_rate=22050, hop_length=256)
    assert inspect.signature(fs2amd.f0_contour).parameters["method"].default == "yin"
    assert inspect.signature(fs2amd.build_corpus).parameters["f0_method"].default == "yin"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.f0_contour([np.zeros(100, dtype=np.int16)], sampling_rate=22050, hop_length=256, method="track", device="cpu")
    assert lib.OPS_F0_TRACK == ("f0_track",) and hasattr(torch.ops.fs2, "f0_track")
    assert not set(lib.OPS_F0_TRACK) & (set(lib.OPS) | set(lib.OPS_PREP) | set(lib.OPS_F0) | set(lib.OPS_EVAL))
    with FakeTensorMode():
        cmnd = torch.empty(3, 20, 312, device="cuda", dtype=torch.float64)
        f0, state, score = torch.ops.fs2.f0_track(cmnd, None, 22050.0, 256, 71.0, 800.0, 5, 12, 0.01)
        assert f0.shape == state.shape == (3, 20) and score.shape == (3,)
        assert f0.dtype == score.dtype == torch.float64 and state.dtype == torch.int32
