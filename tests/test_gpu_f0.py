"""F0 estimation on the GPU (include/fs2hip_f0.h, ops.f0_yin, fs2amd.preprocess.f0_contour) against
the numpy restatement of tests/_f0.py and the contours stored in tests/golden/f0_a.npz.

int16 input (and float32 samples that are k * 2^-15) is exact in any summation order: f0, tau and
the whole cmnd table are compared bit for bit. General float32 input: every cmnd entry within the
header's bound FS2_F0_DP_ULPS(W, tau) * 2^-53 (relative) of the restatement's, and f0 / tau bit for
bit what the restatement's pick gives on the GPU's own table."""
import filecmp
import os

import numpy as np
import pytest
import torch

import _f0 as Y

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
KW = dict(sampling_rate=Y.SR, hop_length=Y.HOP, win_length=Y.WIN)
KW200 = dict(sampling_rate=Y.SR, hop_length=200, win_length=800)


@pytest.fixture(scope="module")
def fx():
    return Y.load_fixture()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def launch(wav, lens, **kw):
    from fs2amd import ops

    o = ops.f0_yin(dev(wav), torch.from_numpy(np.asarray(lens, dtype=np.int64)), want_cmnd=True, **kw)
    return o.f0.cpu().numpy(), o.tau.cpu().numpy(), o.cmnd.cpu().numpy()


@pytest.fixture(scope="module")
def run16(fx):
    """Every int16 case of the fixture in one batched launch."""
    return launch(fx["wav16"], fx["lens16"], **KW)


@pytest.fixture(scope="module")
def run32(fx):
    return launch(fx["wav32"], fx["lens32"], **KW)


def check_exact(wav, lens, got, ref_f0, ref_tau, hop, W):
    f0, tau, cmnd = got
    F_max = wav.shape[1] // hop + 1
    assert f0.shape == tau.shape == (len(lens), F_max) and cmnd.shape == (len(lens), F_max, Y.lags()[1] + 1)
    same_bits(f0, ref_f0)
    same_bits(tau, ref_tau)
    for b, n in enumerate(lens):
        F = Y.n_frames(int(n), hop)
        same_bits(cmnd[b, :F], Y.table(wav[b, :n], hop, W)[1])
        assert (bits(cmnd[b, F:]) == 0).all() and (bits(f0[b, F:]) == 0).all() and (tau[b, F:] == 0).all()


def test_int16_cases_are_the_fixtures_bits(fx, run16):
    check_exact(fx["wav16"], fx["lens16"], run16, fx["f0_16"], fx["tau_16"], Y.HOP, Y.WIN)


def test_hop_that_is_no_power_of_two(fx):
    got = launch(fx["wav200"], fx["lens200"], **KW200)
    check_exact(fx["wav200"], fx["lens200"], got, fx["f0_200"], fx["tau_200"], 200, 800)


def test_float32_twin_of_an_int16_case_gives_the_same_bits(fx, run16, run32):
    twin, F_max = int(fx["twin16"]), run32[0].shape[1]
    same_bits(run32[0][0], run16[0][twin, :F_max])
    same_bits(run32[1][0], run16[1][twin, :F_max])
    same_bits(run32[2][0], run16[2][twin, :F_max])  # dp is scale-free: the table too
    same_bits(run32[0][0], fx["f0_32"][0])


def test_general_float32_case_is_within_the_headers_bound(fx, run32):
    from fs2amd import _lib

    n = int(fx["lens32"][1])
    F, tau_max = Y.n_frames(n, Y.HOP), Y.lags()[1]
    f0, tau, cmnd = (r[1] for r in run32)
    ref = Y.table(fx["wav32"][1, :n])[1]
    bound = np.array([_lib.f0_dp_ulps(Y.WIN, t) for t in range(tau_max + 1)]) * Y.U
    rel = np.abs(cmnd[:F] - ref) / np.abs(ref)
    print(f"general float32: max |cmnd - restatement| / bound = {(rel / bound[None, :]).max():.3e}")
    assert (rel <= bound[None, :]).all()
    own_f0, own_tau = Y.contour_of_table(cmnd[:F])
    same_bits(f0[:F], own_f0)
    same_bits(tau[:F], own_tau)
    np.testing.assert_array_equal(tau[:F], fx["tau_32"][1, :F])  # no fragile frame (tests/test_f0_host.py)
    assert (bits(f0[F:]) == 0).all() and (tau[F:] == 0).all() and (bits(cmnd[F:]) == 0).all()


def test_without_tau_and_cmnd_the_contour_is_the_same(fx, run16, run32):
    from fs2amd import ops

    for key, ref in (("16", run16), ("32", run32)):
        o = ops.f0_yin(dev(fx["wav" + key]), torch.from_numpy(fx["lens" + key]), want_tau=False, **KW)
        assert o.tau is None and o.cmnd is None
        same_bits(o.f0.cpu().numpy(), ref[0])


def test_an_utterance_does_not_depend_on_its_batch(fx, run16):
    from fs2amd import ops

    names = list(fx["names16"])
    for name in ("splice_a", "tone220_1335"):
        b = names.index(name)
        n = int(fx["lens16"][b])
        F = Y.n_frames(n, Y.HOP)
        w = fx["wav16"][b, :max(n, 1)]
        alone = launch(w[None, :], [n], **KW)
        first = launch(np.stack([fx["wav16"][b], fx["wav16"][3], fx["wav16"][10]]), [n, fx["lens16"][3], fx["lens16"][10]],
                       **KW)
        # last in a wider batch: a larger n_max and a row stride beyond it, rubbish past the length
        buf = torch.full((4, 12000), 12345, dtype=torch.int16, device=DEV)
        view = buf[:, :11000]
        view[:3, :fx["wav16"].shape[1]] = dev(fx["wav16"][:3])
        view[3, :n] = dev(fx["wav16"][b, :n])
        lens = torch.tensor([int(fx["lens16"][0]), int(fx["lens16"][1]), int(fx["lens16"][2]), n])
        o = ops.f0_yin(view, lens, want_cmnd=True, **KW)
        last = (o.f0[3].cpu().numpy(), o.tau[3].cpu().numpy(), o.cmnd[3].cpu().numpy())
        for k in range(3):
            same_bits(alone[k][0][:F], run16[k][b, :F])
            same_bits(first[k][0][:F], run16[k][b, :F])
            same_bits(last[k][:F], run16[k][b, :F])
            assert (bits(last[k][F:]) == 0).all()


def test_nothing_outside_the_extents_is_written_and_nothing_inside_left(fx, run16):
    from fs2amd import ops

    wav, lens = fx["wav16"], fx["lens16"]
    B, F_max, T = wav.shape[0], wav.shape[1] // Y.HOP + 1, Y.lags()[1] + 1
    nan = float("nan")
    fbuf = torch.full((GUARD + B * F_max + GUARD,), nan, dtype=torch.float64, device=DEV)
    tbuf = torch.full((GUARD + B * F_max + GUARD,), -7, dtype=torch.int32, device=DEV)
    cbuf = torch.full((GUARD + B * F_max * T + GUARD,), nan, dtype=torch.float64, device=DEV)
    f0 = fbuf[GUARD:GUARD + B * F_max].view(B, F_max)
    tau = tbuf[GUARD:GUARD + B * F_max].view(B, F_max)
    cmnd = cbuf[GUARD:GUARD + B * F_max * T].view(B, F_max, T)
    ops.f0_yin(dev(wav), torch.from_numpy(lens), out=(f0, tau, cmnd), **KW)
    for buf, inner in ((fbuf, f0), (cbuf, cmnd)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all() and not torch.isnan(inner).any()
    assert (tbuf[:GUARD] == -7).all() and (tbuf[-GUARD:] == -7).all() and (tau >= 0).all()
    same_bits(f0.cpu().numpy(), run16[0])
    same_bits(tau.cpu().numpy(), run16[1])
    same_bits(cmnd.cpu().numpy(), run16[2])


def test_f0_contour_returns_the_rows(fx, run16):
    import fs2amd

    wavs = Y.ragged(fx, "wav16", "lens16")
    got = fs2amd.f0_contour(wavs, sampling_rate=22050, hop_length=256, device=DEV)
    assert len(got) == len(wavs)
    for b, (w, f0) in enumerate(zip(wavs, got)):
        assert f0.dtype == np.float64 and f0.shape == (len(w) // 256 + 1,)
        same_bits(f0, run16[0][b, :len(f0)])
    assert fs2amd.f0_contour([], sampling_rate=22050, hop_length=256, device=DEV) == []
    # another range: the lags follow it
    low = fs2amd.f0_contour(wavs[9:11], sampling_rate=22050, hop_length=256, f0_ceil=400.0, device=DEV)
    for w, f0 in zip(wavs[9:11], low):
        same_bits(f0, Y.contour(w, f0_ceil=400.0)[0])


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_build_corpus_estimates_the_contours_it_is_not_given(tmp_path):
    import fs2amd
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "a"))
    utts = _utterances(np.random.default_rng(5))
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    f0s = fs2amd.f0_contour([u["wav"] for u in utts], sampling_rate=22050, hop_length=256, device=DEV)
    assert all(len(f) == len(u["wav"]) // 256 + 1 and (f[4:-4] > 0).mean() > 0.5 for f, u in zip(f0s, utts))
    variants = {
        "given": [dict(u, f0=f) for u, f in zip(utts, f0s)],
        "absent": [{k: v for k, v in u.items() if k != "f0"} for u in utts],
        "mixed": [dict(u, f0=(f if i % 2 else None)) for i, (u, f) in enumerate(zip(utts, f0s))],
    }
    lines = {}
    for tag, us in variants.items():
        lines[tag] = fs2amd.build_corpus(str(tmp_path / tag), us, pc, stft=stft, val_size=2, seed=1234, batch_size=4,
                                         emotions=SYNTH_EMOTIONS)
    files = _tree(str(tmp_path / "given"))
    assert len(lines["given"]) == 6 and len(files) == 4 * 6 + 5
    for tag in ("absent", "mixed"):
        assert lines[tag] == lines["given"] and _tree(str(tmp_path / tag)) == files
        match, mismatch, errors = filecmp.cmpfiles(str(tmp_path / "given"), str(tmp_path / tag), files, shallow=False)
        assert not mismatch and not errors and len(match) == len(files), (tag, mismatch, errors)
    # the optional sub-dict: the defaults spelled out change nothing, another range does
    pp = dict(pc["preprocessing"], pitch_extraction={"f0_floor": 71.0, "f0_ceil": 800.0, "threshold": 0.1,
                                                     "win_length": 1024})
    fs2amd.build_corpus(str(tmp_path / "spelled"), variants["absent"], dict(pc, preprocessing=pp), stft=stft, val_size=2,
                        seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)
    assert not filecmp.cmpfiles(str(tmp_path / "given"), str(tmp_path / "spelled"), files, shallow=False)[1]
    pp = dict(pc["preprocessing"], pitch_extraction={"f0_floor": 160.0})
    fs2amd.build_corpus(str(tmp_path / "narrow"), variants["absent"], dict(pc, preprocessing=pp), stft=stft, val_size=2,
                        seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)
    assert open(str(tmp_path / "narrow" / "stats.json")).read() != open(str(tmp_path / "given" / "stats.json")).read()
