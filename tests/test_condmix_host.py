"""Mixture / curve conditioning without a GPU: the fs2amd.emotion helpers, FS2_EINVAL for every
status row of include/fs2hip_cond_mix.h through the loaded library, the ValueErrors and the launch
sequences of the two new forms on the stubbed library (the dry-run pattern of test_host.py), and the
committed fixtures."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from _common import GOLDEN, configs
from _npz_parts import load_npz_parts
from _stubs import RecordingLib

EMO = {"Angry": 0, "Happy": 1, "Neutral": 2, "Sad": 3, "Surprise": 4}
ARO = {"0.3": 0, "0.5": 1, "0.8": 2, "0.9": 3}


# ---- fs2amd.emotion ---------------------------------------------------------------------------------
def test_helpers_are_exported():
    import fs2amd
    from fs2amd import emotion

    for name in ("mixture", "level_weights", "curve", "one_hot"):
        assert getattr(fs2amd, name) is getattr(emotion, name) and name in fs2amd.__all__


def test_mixture_and_one_hot():
    from fs2amd import mixture, one_hot

    w = mixture({"Happy": .7, "Neutral": .3}, EMO)
    assert w.dtype == torch.float32 and w.tolist() == pytest.approx([0, .7, .3, 0, 0])
    assert mixture({"Sad": 1.4, "Angry": -0.2}, EMO).tolist() == pytest.approx([-0.2, 0, 0, 1.4, 0])  # as given
    with pytest.raises(KeyError, match="Joy"):
        mixture({"Joy": 1.0}, EMO)
    h = one_hot(torch.tensor([3, 0]), 5)
    assert h.dtype == torch.float32 and h.tolist() == [[0, 0, 0, 1, 0], [1, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        one_hot([5], 5)


def test_level_weights_at_between_and_outside_levels():
    from fs2amd import level_weights

    assert level_weights(0.5, ARO).tolist() == [0, 1, 0, 0]                      # at a level
    assert level_weights(0.65, ARO).tolist() == pytest.approx([0, .5, .5, 0])    # between 0.5 and 0.8
    assert level_weights(0.35, ARO).tolist() == pytest.approx([.75, .25, 0, 0])
    assert level_weights(0.1, ARO).tolist() == [1, 0, 0, 0]                      # clamped below
    assert level_weights(2.0, ARO).tolist() == [0, 0, 0, 1]                      # clamped above
    # rows follow the dictionary's values, not the order of its keys
    assert level_weights(0.8, {"0.8": 0, "0.2": 1}).tolist() == [1, 0]
    assert level_weights(0.5, {"0.8": 0, "0.2": 1}).tolist() == pytest.approx([.5, .5])


def test_curve_at_between_and_beyond_keyframes():
    from fs2amd import curve, mixture

    a, b = mixture({"Neutral": 1}, EMO), mixture({"Angry": 1}, EMO)
    c = curve([(2, a), (6, b)], src_len=8, L=11)
    assert c.shape == (11, 5) and c.dtype == torch.float32
    assert torch.equal(c[0], a) and torch.equal(c[2], a)          # before / at the first keyframe
    assert torch.equal(c[6], b) and torch.equal(c[7], b)          # at / after the last one
    assert c[4].tolist() == pytest.approx([.5, 0, .5, 0, 0])      # half way
    assert c[3].tolist() == pytest.approx([.25, 0, .75, 0, 0])
    assert all(torch.equal(c[i], c[7]) for i in range(8, 11))     # beyond src_len: the last valid position
    c2 = curve([(0, a), (9, b)], src_len=4, L=6)                  # a keyframe past src_len is never reached
    assert torch.equal(c2[4], c2[3]) and torch.equal(c2[5], c2[3]) and c2[3].tolist() == pytest.approx(
        [1 / 3, 0, 2 / 3, 0, 0])
    with pytest.raises(ValueError):
        curve([], 3, 3)
    with pytest.raises(ValueError):
        curve([(1, a), (1, b)], 3, 3)


# ---- the C ABI's argument checks ---------------------------------------------------------------------
def _desc(_lib, **over):
    """A descriptor every check accepts (dummy non-NULL pointers: nothing is launched before the
    checks pass, and no test below lets them pass with B > 0)."""
    d = _lib.CondMixDesc()
    p = 256
    d.speakers, d.spk_kind, d.speaker_table, d.n_speaker = p, _lib.COND_MIX, p, 10
    d.emotions, d.emo_kind, d.emo_table, d.n_emo, d.d_emo = p, _lib.COND_MIX, p, 5, 128
    d.arousals, d.aro_kind, d.aro_table, d.n_aro, d.d_aro = p, _lib.COND_IDS, p, 4, 64
    d.valences, d.val_kind, d.val_table, d.n_val, d.d_val = p, _lib.COND_MIX, p, 5, 64
    d.lin_w, d.lin_b, d.B, d.D, d.spk_out, d.emo_out = p, p, 0, 256, p, p
    for k, v in over.items():
        setattr(d, k, v)
    return d


EMO_ROWS = [dict(emo_kind=0), dict(aro_kind=7), dict(val_kind=-1), dict(emotions=None), dict(arousals=None),
            dict(valences=None), dict(aro_table=None), dict(val_table=None), dict(lin_w=None), dict(lin_b=None),
            dict(n_emo=0), dict(n_aro=0), dict(n_val=-1), dict(d_emo=0), dict(d_aro=0), dict(d_val=-3)]


def test_cond_mix_rejects_every_status_row_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    call = lambda **over: lib.fs2_cond_mix(ctypes.byref(_desc(_lib, **over)), None)
    assert lib.fs2_cond_mix(None, None) == _lib.FS2_EINVAL                                         # row 1
    assert call(B=-1) == _lib.FS2_EINVAL and call(D=0) == _lib.FS2_EINVAL                          # row 2
    for over in (dict(spk_kind=_lib.COND_NONE), dict(spk_kind=_lib.COND_ROWS), dict(speakers=None),
                 dict(spk_out=None), dict(n_speaker=0)):                                           # row 3
        assert call(**over) == _lib.FS2_EINVAL, over
    for over in EMO_ROWS + [dict(emo_kind=_lib.COND_ROWS), dict(val_kind=_lib.COND_ROWS), dict(emo_out=None)]:
        assert call(**over) == _lib.FS2_EINVAL, over                                               # rows 4-6
    assert call(B=1, d_emo=2000) == _lib.FS2_EUNSUPPORTED
    # nothing to do: B == 0, or neither table (the other fields are then not looked at)
    assert call() == _lib.FS2_OK
    assert call(B=4, speaker_table=None, emo_table=None, speakers=None, lin_w=None) == _lib.FS2_OK


def test_cond_mix_rows_rejects_every_status_row_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    call = lambda L=4, x=256, dt=_lib.FS2_BF16, **over: lib.fs2_cond_mix_rows(
        ctypes.byref(_desc(_lib, **dict(dict(emo_kind=_lib.COND_ROWS), **over))), L, x, dt, None)
    assert lib.fs2_cond_mix_rows(None, 4, 256, _lib.FS2_F32, None) == _lib.FS2_EINVAL               # row 1
    assert call(x=None) == _lib.FS2_EINVAL
    assert call(B=-1) == _lib.FS2_EINVAL and call(L=-1) == _lib.FS2_EINVAL and call(D=0) == _lib.FS2_EINVAL  # 2
    assert call(emo_table=None) == _lib.FS2_EINVAL                                                  # row 3
    for over in EMO_ROWS:                                                                           # rows 4-6
        assert call(**over) == _lib.FS2_EINVAL, over
    assert call(dt=_lib.FS2_FP8) == _lib.FS2_EUNSUPPORTED
    assert call(d_emo=700) == _lib.FS2_EUNSUPPORTED
    assert call(B=1 << 16, L=1 << 15) == _lib.FS2_EUNSUPPORTED                                      # B * L = 2^31
    # nothing to do: B * L == 0; the speaker fields and the outputs are not read
    assert call() == _lib.FS2_OK and call(B=3, L=0) == _lib.FS2_OK
    assert call(speakers=None, spk_kind=0, speaker_table=None, spk_out=None, emo_out=None) == _lib.FS2_OK


def test_bindings_and_header():
    from fs2amd import _lib

    assert set(_lib.SIGNATURES_COND_MIX) == {"fs2_cond_mix", "fs2_cond_mix_rows"}
    assert "fs2hip_cond_mix.h" in _lib.EXTRA_HEADERS and len(_lib.SIGNATURES) == 71
    declared = _lib.header_symbols(_lib.HEADER_COND_MIX)
    assert declared == sorted(_lib.SIGNATURES_COND_MIX), declared
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    text = open(_lib.HEADER_COND_MIX).read()
    for name, val in (("NONE", _lib.COND_NONE), ("IDS", _lib.COND_IDS), ("MIX", _lib.COND_MIX), ("ROWS", _lib.COND_ROWS)):
        assert f"#define FS2_COND_{name} {val}\n" in text
    import __graft_entry__ as G

    assert "cond_mix.hip" in G.HIP_SOURCES


# ---- the forward on the stubbed library ---------------------------------------------------------------
class _FakeForkJoin:
    def __init__(self, dev, n):
        self.n = n
        self.ctx = lambda i: contextlib.nullcontext()

    def fork(self):
        pass

    def join(self, *t):
        pass


@pytest.fixture
def dry(monkeypatch):
    """(model, recording library): FastSpeech2.forward on CPU tensors with the kernels stubbed."""
    from fs2amd import _lib, ops, runtime
    from fs2amd.model import FastSpeech2

    rec = RecordingLib(_lib.load())
    monkeypatch.setattr(ops, "_lib", rec)
    monkeypatch.setattr(ops, "_gpu", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda *a: None)
    monkeypatch.setattr(runtime, "_device_ok", lambda dev: True)
    monkeypatch.setattr(runtime, "_ForkJoin", _FakeForkJoin)
    monkeypatch.setenv("FS2_PACKED_DECODER", "0")
    monkeypatch.setattr(ops, "len_stats", lambda lens, bad=None: torch.stack(
        [lens.max(), lens.sum(), torch.zeros((), dtype=lens.dtype)]).to(torch.int32))
    real_lr = ops.lr_durations

    def lr_durations(dur, logpred=False, d_control=1.0):  # the stubbed kernel writes nothing
        cum, ml, dr = real_lr(dur, logpred, d_control)
        ml.fill_(7)
        return cum, ml, dr

    monkeypatch.setattr(ops, "lr_durations", lr_durations)
    pc, mc, _ = configs()
    return FastSpeech2(pc, mc).eval(), rec


def _batch(B=17, seed=2):
    from fs2amd.data import synth_batch

    return synth_batch(B, 6, 11, seed=seed, teacher=False)


def _hot(args, name, n, L=None):
    w = torch.nn.functional.one_hot(args[name], n).float()
    return w if L is None else w[:, None, :].expand(-1, L, -1).contiguous()


N = {"speakers": 10, "emotions": 5, "arousals": 4, "valences": 5}


@pytest.mark.parametrize("streams", ["1", "2"])
def test_launch_sequence_of_ids_mixtures_and_curves(dry, monkeypatch, streams):
    model, rec = dry
    monkeypatch.setenv("FS2_STREAMS", streams)
    k = int(streams)
    args = _batch()
    L = args["max_src_len"]
    with torch.no_grad():
        out = model(**args)
        assert len(out) == 10 and rec.calls.count("fs2_cond_vectors") == k
        assert not any(c.startswith("fs2_cond_mix") for c in rec.calls)        # the id path is what it was
        del rec.calls[:]
        out = model(**dict(args, emotions=_hot(args, "emotions", 5), speakers=_hot(args, "speakers", 10)))
        assert len(out) == 10 and out[0].shape[0] == args["texts"].shape[0]
        assert rec.calls.count("fs2_cond_mix") == k and "fs2_cond_vectors" not in rec.calls
        assert "fs2_cond_mix_rows" not in rec.calls
        del rec.calls[:]
        out = model(**dict(args, arousals=_hot(args, "arousals", 4, L)))
        assert len(out) == 10
        assert rec.calls.count("fs2_cond_mix_rows") == k and "fs2_cond_vectors" not in rec.calls
        assert rec.calls.count("fs2_cond_mix") == k                            # the speaker vector
        # the curve is added after the encoder stack (4 blocks x 4 GEMMs) and before the predictors
        per = len(rec.calls) // k
        i = rec.calls.index("fs2_cond_mix_rows")
        assert rec.calls[:i].count("fs2_conv1d") == 16 and rec.calls[:per].count("fs2_conv1d") > 16


def test_value_errors(dry):
    model, rec = dry
    args = _batch()
    B, L = args["texts"].shape
    bad = {
        "wrong n": dict(emotions=torch.ones(B, 4)),
        "wrong B": dict(arousals=torch.ones(B + 1, 4)),
        "wrong L": dict(valences=torch.ones(B, L + 1, 5)),
        "wrong n in a curve": dict(emotions=torch.ones(B, L, 6)),
        "float ids": dict(emotions=args["emotions"].float()),
        "rank 4": dict(arousals=torch.ones(B, L, 4, 1)),
        "speaker curve": dict(speakers=torch.ones(B, L, 10)),
        "float64 of the wrong shape": dict(valences=torch.ones(B, 3, dtype=torch.float64)),
    }
    for what, over in bad.items():
        with pytest.raises(ValueError):
            with torch.no_grad():
                model(**dict(args, **over))
        assert not rec.calls, what  # raised before any launch
    with torch.no_grad():  # other floating dtypes are weights too (cast to f32)
        model(**dict(args, valences=_hot(args, "valences", 5).double()))
    assert "fs2_cond_mix" in rec.calls


def test_training_mode_refuses_weights():
    from fs2amd.data import synth_batch
    from fs2amd.model import FastSpeech2

    pc, mc, _ = configs()
    m = FastSpeech2(pc, mc).train()
    args = synth_batch(2, 8, seed=3, with_mels=True, pe_targets=True)
    for name in ("speakers", "emotions", "arousals", "valences"):
        with pytest.raises(ValueError, match="training"):
            m(**dict(args, **{name: _hot(args, name, N[name])}))


def test_cond_inputs_classifies():
    from types import SimpleNamespace

    from fs2amd import runtime as R

    P = SimpleNamespace(spk_table=torch.zeros(10, 8), emo_table=torch.zeros(5, 4), aro_table=torch.zeros(4, 2),
                        val_table=torch.zeros(5, 2))
    ids = torch.tensor([1, 2, 3], dtype=torch.int32)
    t, forms = R.cond_inputs(P, ids, torch.ones(3, 5, dtype=torch.float64), torch.ones(3, 7, 4)[:, :, :], [0, 1, 2],
                             3, 7, "cpu")
    assert forms == ("ids", ("mix", 5), ("curve", 4), "ids")
    assert t["speakers"].dtype == torch.int64 and t["valences"].dtype == torch.int64
    assert t["emotions"].dtype == torch.float32 and t["arousals"].is_contiguous()
    # a model without the table never reads the input
    P2 = SimpleNamespace(spk_table=None, emo_table=None)
    t, forms = R.cond_inputs(P2, torch.ones(3, 10), ids, ids, ids, 3, 7, "cpu")
    assert forms == R.ALL_IDS and t["speakers"] is None


# ---- fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,curves", [("condmix_a", False), ("condmix_b", True)])
def test_fixtures_load_and_margins_hold(name, curves):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) < 1 << 20
    z = load_npz_parts(path)
    B, L = z["in_texts"].shape
    assert B == 3 and L == int(z["in_max_src_len"]) == z["in_src_lens"].max() and L == (17 if curves else 13)
    assert z["out_mel"].shape == z["out_postnet_mel"].shape
    for k in ("speakers", "emotions", "arousals", "valences"):
        w = z["w_" + k]
        if w.dtype.kind == "f":
            assert w.dtype == np.float32 and w.shape[0] == B and w.shape[-1] == N[k] and np.isfinite(w).all()
        else:
            np.testing.assert_array_equal(w, z["in_" + k])
    if curves:
        assert z["w_emotions"].shape == (B, L, 5) and z["w_arousals"].shape == (B, 4) and z["w_valences"].ndim == 1
        w = z["w_arousals"].astype(np.float64)
    else:
        assert all(z["w_" + k].ndim == 2 for k in N)
        w = z["w_emotions"].astype(np.float64)
    # normalised rows, one row of sum 1.4, one row with a negative entry
    assert abs(w[0].sum() - 1) < 1e-6 and abs(w[1].sum() - 1.4) < 1e-6 and w[2].min() < 0 and w[:2].min() > 0
    # the stored outputs sit clear of every discrete decision
    valid = ~z["out_src_masks"]
    edge = lambda v, bins: float(np.abs(v.astype(np.float64)[valid][:, None] - bins.astype(np.float64)[None, :]).min())
    d = np.exp(z["out_log_d"].astype(np.float32))[valid].astype(np.float64) - 1.0
    got = (edge(z["out_p_pred"], z["pitch_bins"]), edge(z["out_e_pred"], z["energy_bins"]),
           float(np.abs(d - np.floor(d) - 0.5).min()))
    assert got == pytest.approx(tuple(z["margins"]), rel=1e-9)
    assert got[0] >= 1e-3 and got[1] >= 1e-3 and got[2] >= 6e-3, got
    np.testing.assert_array_equal(np.round(np.clip(d, 0, None)), z["out_d_rounded"][valid])
