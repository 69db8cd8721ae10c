"""F0 tracking on the GPU (include/fs2hip_f0_track.h, ops.f0_track, f0_contour(method="track"),
build_corpus(f0_method="track")) against the numpy restatement of tests/_f0_track.py and the paths
stored in tests/golden/f0_track_a.npz.

The tracker only compares, adds and looks up, so given the dp table everything is compared bit for
bit: on int16 input (where the table itself is exact) against the fixture, on general float32 input
against the restatement run on the GPU's own table."""
import copy
import filecmp
import json
import os

import numpy as np
import pytest
import torch

import _f0 as Y
import _f0_track as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
KW = dict(sampling_rate=Y.SR, hop_length=Y.HOP)
YKW = dict(KW, win_length=Y.WIN)


@pytest.fixture(scope="module")
def fx():
    return T.load_fixture()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def launch(wav, lens, hop=Y.HOP, W=Y.WIN, **kw):
    """ops.f0_yin with its cmnd table, then ops.f0_track over it: (f0, state, score, cmnd) on the host."""
    from fs2amd import ops

    lens = torch.from_numpy(np.asarray(lens, dtype=np.int64))
    cmnd = ops.f0_yin(dev(wav), lens, sampling_rate=Y.SR, hop_length=hop, win_length=W, want_cmnd=True).cmnd
    o = ops.f0_track(cmnd, lens, sampling_rate=Y.SR, hop_length=hop, **kw)
    return o.f0.cpu().numpy(), o.state.cpu().numpy(), o.score.cpu().numpy(), cmnd.cpu().numpy()


@pytest.fixture(scope="module")
def run16(fx):
    """Every int16 case of the fixture in one batched launch."""
    return launch(fx["wav16"], fx["lens16"])


@pytest.fixture(scope="module")
def run32(fx):
    return launch(fx["wav32"], fx["lens32"])


def check_exact(wav, lens, got, ref, hop):
    f0, state, score, _ = got
    F_max = wav.shape[1] // hop + 1
    assert f0.shape == state.shape == (len(lens), F_max) and score.shape == (len(lens),)
    same_bits(f0, ref[0])
    same_bits(state, ref[1])
    same_bits(score, ref[2])
    for b, n in enumerate(lens):
        F = Y.n_frames(int(n), hop)
        assert (bits(f0[b, F:]) == 0).all() and (state[b, F:] == -1).all()


def test_int16_cases_are_the_fixtures_bits(fx, run16):
    check_exact(fx["wav16"], fx["lens16"], run16, (fx["f0_16"], fx["state_16"], fx["score_16"]), Y.HOP)
    names = list(fx["names16"])
    for name in ("trap", "weak"):  # what plain YIN gets wrong on the same table, the path does not
        b = names.index(name)
        F = Y.n_frames(int(fx["lens16"][b]), Y.HOP)
        sl = slice(T.MARGIN, F - T.MARGIN)
        assert not T.wrong(run16[0][b, :F][sl], fx["truth16"][b, :F][sl]).any()
        assert T.wrong(Y.contour_of_table(run16[3][b, :F])[0][sl], fx["truth16"][b, :F][sl]).any()


def test_hop_that_is_no_power_of_two(fx):
    got = launch(fx["wav200"], fx["lens200"], hop=200, W=800)
    check_exact(fx["wav200"], fx["lens200"], got, (fx["f0_200"], fx["state_200"], fx["score_200"]), 200)


def test_float32_twin_of_an_int16_case_gives_the_same_bits(fx, run16, run32):
    twin, F_max = int(fx["twin16"]), run32[0].shape[1]
    same_bits(run32[0][0], run16[0][twin, :F_max])
    same_bits(run32[1][0], run16[1][twin, :F_max])
    same_bits(run32[2][0], run16[2][twin])
    same_bits(run32[0][0], fx["f0_32"][0])


def test_general_float32_case_is_the_restatement_on_the_gpus_own_table(fx, run32):
    n = int(fx["lens32"][1])
    F = Y.n_frames(n, Y.HOP)
    f0, state, score, cmnd = (r[1] for r in run32)
    r_f0, r_state, r_score, _, _, _ = T.track_table(cmnd[:F], T.tables())
    same_bits(f0[:F], r_f0)
    same_bits(state[:F], r_state)
    same_bits(score, np.float64(r_score))
    np.testing.assert_array_equal(state[:F], fx["state_32"][1, :F])  # no fragile comparison (tests/test_f0_track_host.py)
    assert (bits(f0[F:]) == 0).all() and (state[F:] == -1).all()


def tie_tables():
    """The package's tables of T.TIE_PARAMS with the integer overrides of T.tie_overrides."""
    from fs2amd.f0 import f0_track_tables

    p = T.TIE_PARAMS
    pk = copy.copy(f0_track_tables(p["sr"], p["f0_floor"], p["f0_ceil"], p["bins_per_semitone"], p["max_step"], 0.01))
    for k, v in T.tie_overrides(pk.n_bins, pk.max_step).items():
        setattr(pk, k, v)
    pk._dev = {}
    return pk


def test_tie_order_on_the_hand_built_table():
    from fs2amd import ops

    tb, cmnd = T.tie_case()
    r_f0, r_state, r_score, _, ties, final_tie = T.track_table(cmnd, tb)
    assert ties.any() and final_tie
    p = T.TIE_PARAMS
    # twice in one batch, the second cut short: lens in samples, hop 10
    batch = np.stack([cmnd, cmnd])
    o = ops.f0_track(dev(batch), torch.tensor([40, 25]), sampling_rate=p["sr"], hop_length=10, f0_floor=p["f0_floor"],
                     f0_ceil=p["f0_ceil"], tables=tie_tables())
    same_bits(o.f0[0].cpu().numpy(), r_f0)
    same_bits(o.state[0].cpu().numpy(), r_state)
    assert o.score[0].item() == r_score == -1.0
    np.testing.assert_array_equal(o.state[0].cpu().numpy(), np.full(5, 12, dtype=np.int32))  # the lower bin of the tied pair
    s_f0, s_state, s_score, _, _, _ = T.track_table(cmnd[:3], tb)
    same_bits(o.f0[1, :3].cpu().numpy(), s_f0)
    same_bits(o.state[1].cpu().numpy(), np.concatenate([s_state, [-1, -1]]).astype(np.int32))
    assert o.score[1].item() == s_score and (o.f0[1, 3:] == 0).all()


def test_an_utterance_does_not_depend_on_its_batch(fx, run16):
    from fs2amd import ops

    names = list(fx["names16"])
    T1 = Y.lags()[1] + 1
    for name in ("splice", "tone220_1335"):
        b = names.index(name)
        n = int(fx["lens16"][b])
        F = Y.n_frames(n, Y.HOP)
        table = run16[3][b]
        alone = ops.f0_track(dev(table[None, :F]), torch.tensor([n]), **KW)
        # first and last in a wider batch: a larger F_max, so other strides, rubbish (NaN) past the lengths
        wide = torch.full((4, 50, T1), float("nan"), dtype=torch.float64, device=DEV)
        wide[0, :F] = dev(table[:F])
        wide[3, :F] = dev(table[:F])
        other = names.index("weak")
        wide[1, :36] = dev(run16[3][other, :36])
        wide[2, :12] = dev(run16[3][names.index("noise"), :12])
        lens = torch.tensor([n, int(fx["lens16"][other]), 3000, n])
        o = ops.f0_track(wide, lens, **KW)
        for got_f0, got_state, got_score in ((alone.f0[0], alone.state[0], alone.score[0]), (o.f0[0], o.state[0], o.score[0]),
                                             (o.f0[3], o.state[3], o.score[3])):
            same_bits(got_f0[:F].cpu().numpy(), run16[0][b, :F])
            same_bits(got_state[:F].cpu().numpy(), run16[1][b, :F])
            same_bits(got_score.cpu().numpy(), run16[2][b])
            assert (bits(got_f0[F:].cpu().numpy()) == 0).all() and (got_state[F:] == -1).all()
        same_bits(o.f0[1, :36].cpu().numpy(), run16[0][other, :36])


def test_nothing_outside_the_extents_is_written_and_nothing_inside_left(fx, run16):
    from fs2amd import _lib, ops

    lens = fx["lens16"]
    cmnd = dev(run16[3])
    B, F_max = cmnd.shape[0], cmnd.shape[1]
    tau_min, tau_max = Y.lags()
    need = _lib.f0_track_workspace_bytes(B, F_max, tau_min, tau_max, 210)
    assert need == _lib.load().fs2_f0_track_workspace_bytes(B, F_max, tau_min, tau_max, 210)
    nan = float("nan")
    fbuf = torch.full((GUARD + B * F_max + GUARD,), nan, dtype=torch.float64, device=DEV)
    sbuf = torch.full((GUARD + B * F_max + GUARD,), -7, dtype=torch.int32, device=DEV)
    cbuf = torch.full((GUARD + B + GUARD,), nan, dtype=torch.float64, device=DEV)
    wbuf = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    f0 = fbuf[GUARD:GUARD + B * F_max].view(B, F_max)
    state = sbuf[GUARD:GUARD + B * F_max].view(B, F_max)
    score = cbuf[GUARD:GUARD + B]
    ops.f0_track(cmnd, torch.from_numpy(lens), out=(f0, state, score), workspace=wbuf[GUARD:GUARD + need], **KW)
    for buf, inner in ((fbuf, f0), (cbuf, score)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all() and not torch.isnan(inner).any()
    assert (sbuf[:GUARD] == -7).all() and (sbuf[-GUARD:] == -7).all() and (state >= -1).all() and (state < 210).all()
    assert (wbuf[:GUARD] == 0xA5).all() and (wbuf[-GUARD:] == 0xA5).all()
    same_bits(f0.cpu().numpy(), run16[0])
    same_bits(state.cpu().numpy(), run16[1])
    same_bits(score.cpu().numpy(), run16[2])
    # without a score: the same f0 and state
    o = ops.f0_track(cmnd, torch.from_numpy(lens), want_score=False, **KW)
    assert o.score is None
    same_bits(o.f0.cpu().numpy(), run16[0])
    same_bits(o.state.cpu().numpy(), run16[1])
    with pytest.raises(ValueError, match="workspace"):
        ops.f0_track(cmnd, torch.from_numpy(lens), workspace=wbuf[:need - 8], **KW)


def test_entry_point_refuses_what_the_header_says():
    from fs2amd import _lib
    from test_f0_track_host import call_entry, reject_cases

    lib = _lib.load()
    for kw, status in reject_cases():
        assert call_entry(lib, **kw) == status, kw
    from fs2amd import ops

    with pytest.raises(ValueError, match="cmnd"):
        ops.f0_track(torch.zeros(2, 5, 300, dtype=torch.float64, device=DEV), **KW)  # not tau_max + 1 wide
    with pytest.raises(ValueError, match="pitch bins"):
        ops.f0_track(torch.zeros(2, 5, 312, dtype=torch.float64, device=DEV), bins_per_semitone=8, **KW)  # 336 bins


def test_f0_contour_track_is_yin_then_track(fx, run16):
    import fs2amd

    wavs = Y.ragged(fx, "wav16", "lens16")
    got = fs2amd.f0_contour(wavs, sampling_rate=22050, hop_length=256, method="track", device=DEV)
    assert len(got) == len(wavs)
    for b, (w, f0) in enumerate(zip(wavs, got)):
        assert f0.dtype == np.float64 and f0.shape == (len(w) // 256 + 1,)
        same_bits(f0, run16[0][b, :len(f0)])
    assert fs2amd.f0_contour([], sampling_rate=22050, hop_length=256, method="track", device=DEV) == []
    with pytest.raises(ValueError, match="F0 method"):
        fs2amd.f0_contour(wavs[:2], sampling_rate=22050, hop_length=256, method="pyin", device=DEV)
    # the default is plain YIN, as before
    plain = fs2amd.f0_contour(wavs[-2:], sampling_rate=22050, hop_length=256, device=DEV)
    for w, f0 in zip(wavs[-2:], plain):
        same_bits(f0, Y.contour(w)[0])


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_build_corpus_with_the_tracker(tmp_path):
    import fs2amd
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "a"))
    utts = [{k: v for k, v in u.items() if k != "f0"} for u in _utterances(np.random.default_rng(5))]
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    kw = dict(stft=stft, val_size=2, seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)
    wavs = [u["wav"] for u in utts]
    tracked = fs2amd.f0_contour(wavs, sampling_rate=22050, hop_length=256, method="track", device=DEV)
    plain = fs2amd.f0_contour(wavs, sampling_rate=22050, hop_length=256, device=DEV)
    assert any((t != p).any() for t, p in zip(tracked, plain))
    lines = {
        "default": fs2amd.build_corpus(str(tmp_path / "default"), utts, pc, **kw),
        "yin": fs2amd.build_corpus(str(tmp_path / "yin"), utts, pc, f0_method="yin", **kw),
        "parent": fs2amd.build_corpus(str(tmp_path / "parent"), [dict(u, f0=f) for u, f in zip(utts, plain)], pc, **kw),
        "track": fs2amd.build_corpus(str(tmp_path / "track"), utts, pc, f0_method="track", **kw),
        "given": fs2amd.build_corpus(str(tmp_path / "given"), [dict(u, f0=f) for u, f in zip(utts, tracked)], pc, **kw),
    }
    files = _tree(str(tmp_path / "default"))
    assert len(lines["default"]) == 6 and len(files) == 4 * 6 + 5
    assert all(v == lines["default"] and _tree(str(tmp_path / k)) == files for k, v in lines.items())

    def differing(a, b):
        match, mismatch, errors = filecmp.cmpfiles(str(tmp_path / a), str(tmp_path / b), files, shallow=False)
        assert not errors and len(match) + len(mismatch) == len(files)
        return sorted(mismatch)

    # the default is the parent's code path: f0_method left out, spelled out, or the plain contours handed in
    assert differing("default", "yin") == [] and differing("default", "parent") == []
    # the tracker's corpus is the one built from its contours, byte for byte
    assert differing("track", "given") == []
    # and differs from the default only in the pitch entries
    diff = differing("default", "track")
    assert diff and all(f.startswith("pitch" + os.sep) or f == "stats.json" for f in diff), diff
    a, b = (json.load(open(str(tmp_path / k / "stats.json"))) for k in ("default", "track"))
    assert a["energy"] == b["energy"] and a["pitch"] != b["pitch"]
    with pytest.raises(ValueError, match="f0_method"):
        fs2amd.build_corpus(str(tmp_path / "bad"), utts, pc, f0_method="world", **kw)
