"""Per-phoneme control maps through the whole forward (FastSpeech2.forward and SynthGraphs).

* fp32 against the reference's own outputs with [B, L] pitch and duration maps
  (tests/golden/prosody_{a,b}.npz, gen_golden_prosody.py): tolerances are those of
  test_gpu_model.py -- |mel - ref| <= 2e-3, predictions <= 5e-4, every discrete output exact (the
  fixtures sit >= 1e-3 from every bin edge and >= 6e-3 from every rounding tie,
  test_prosody_host.py);
* a constant map equals the scalar call bit for bit (fp32 and bf16, up to the bench shape);
* separate_energy_control; SynthGraphs: one stage-1 graph serves every map.
"""
import numpy as np
import pytest
import torch

from _common import OUT_NAMES, configs, load_case, oracle_state_dict
from _prosody import load_prosody

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd.model import FastSpeech2

    pc, mc, _ = configs()
    m = FastSpeech2(pc, mc)
    m.load_state_dict(oracle_state_dict())
    return m.to(DEV).eval()


def _dev(args):
    from fs2amd.data import to_device

    return to_device(args, DEV)


def _fwd(model, args, **controls):
    with torch.no_grad():
        out = model(**args, **controls)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    for name, x, y in zip(OUT_NAMES, a, b):
        if x is None or y is None:
            assert x is None and y is None, name
            continue
        assert x.shape == y.shape and torch.equal(x, y), name


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


@pytest.mark.parametrize("case", ["prosody_a", "prosody_b"])
def test_fp32_matches_reference_with_maps(model, case):
    from fs2amd import ops

    args, p_map, d_map, outs, z = load_prosody(case)
    model.set_precision("fp32")
    got = _fwd(model, _dev(args), p_control=p_map.to(DEV), e_control=1.0, d_control=d_map.to(DEV))
    for name, g in zip(OUT_NAMES, got):
        ref = outs[name]
        g = _np(g)
        assert g.shape == ref.shape, (case, name, g.shape, ref.shape)
        if name in ("mel", "postnet_mel"):
            err = np.abs(g - ref).max()
            print(f"{case}:{name} max|err| {err:.3e}")
            assert err <= 2e-3, (case, name, err)
        elif name in ("p_pred", "e_pred", "log_d"):
            err = np.abs(g - ref).max()
            print(f"{case}:{name} max|err| {err:.3e}")
            assert err <= 5e-4, (case, name, err)
        elif name == "d_rounded":
            np.testing.assert_array_equal(g.astype(ref.dtype), ref, err_msg=f"{case}:{name}")
        else:  # both masks, src_lens, mel_lens
            np.testing.assert_array_equal(g, ref, err_msg=f"{case}:{name}")
    # the LengthRegulator's source-index map, from the model's own log-durations and the map
    T = int(z["lr_index_map"].shape[1])
    x = torch.zeros(*d_map.shape, 8, device=DEV)
    _, ml, im, dr = ops.length_regulate(x, got[4].contiguous(), T, return_index_map=True, d_control=d_map.to(DEV))
    np.testing.assert_array_equal(_np(im), z["lr_index_map"])
    np.testing.assert_array_equal(_np(ml), z["lr_mel_len"])
    np.testing.assert_array_equal(_np(dr), outs["d_rounded"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["mini_free_ctrl", "cfg2_free"])
def test_constant_map_equals_scalar(model, case, prec):
    """The stored scalars ((1.2, 0.7, 1.3) / (1, 1, 1): the bench shape 64 x 64) passed as [B, L]
    maps: all ten outputs torch.equal to the scalar call."""
    args, (p_c, e_c, d_c), _, _ = load_case(case)
    assert (p_c, d_c) == ((1.2, 1.3) if case == "mini_free_ctrl" else (1.0, 1.0))
    model.set_precision(prec)
    a = _dev(args)
    B, L = a["texts"].shape
    ref = _fwd(model, a, p_control=p_c, e_control=e_c, d_control=d_c)
    got = _fwd(model, a, p_control=torch.full((B, L), p_c, device=DEV), e_control=e_c,
               d_control=torch.full((B, L), d_c, device=DEV))
    _same(got, ref)
    # broadcast forms: [B, 1] and 0-dim
    got = _fwd(model, a, p_control=torch.full((B, 1), p_c, device=DEV), e_control=e_c,
               d_control=torch.tensor(d_c, device=DEV))
    _same(got, ref)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_separate_energy_control(model, prec):
    args, p_map, d_map, outs, _ = load_prosody("prosody_a")
    model.set_precision(prec)
    a = _dev(args)
    P, D = p_map.to(DEV), d_map.to(DEV)
    g = torch.Generator().manual_seed(5)
    E = (0.5 + 1.5 * torch.rand(P.shape, generator=g)).to(DEV)
    va = model.variance_adaptor
    assert va.separate_energy_control is False
    off = _fwd(model, a, p_control=P, e_control=E, d_control=D)  # e_control accepted and ignored
    _same(off, _fwd(model, a, p_control=P, e_control=1.0, d_control=D))
    try:
        va.separate_energy_control = True
        _same(_fwd(model, a, p_control=P, e_control=P, d_control=D), off)
        _same(_fwd(model, a, p_control=P, e_control=P.clone(), d_control=D), off)
        on = _fwd(model, a, p_control=P, e_control=E, d_control=D)
        on_s = _fwd(model, a, p_control=P, e_control=1.25, d_control=D)  # a number for energy alone
    finally:
        va.separate_energy_control = False
    assert torch.equal(on[2], off[2]) and torch.equal(on[5], off[5]) and torch.equal(on[4], off[4])
    assert not torch.equal(on[3], off[3])
    # the energy predictor's input and unscaled output u are the same: e_on = u * E, e_off = u * P,
    # so e_on * P and e_off * E are (u E) P and (u P) E, two roundings each: within 2 ulp
    valid = ~on[6]
    x, y = (on[3] * P)[valid].cpu().numpy(), (off[3] * E)[valid].cpu().numpy()
    assert np.all(np.abs(x - y) <= 2 * np.spacing(np.maximum(np.abs(x), np.abs(y))))
    x, y = (on_s[3] * P)[valid].cpu().numpy(), (off[3] * 1.25)[valid].cpu().numpy()
    assert np.all(np.abs(x - y) <= 2 * np.spacing(np.maximum(np.abs(x), np.abs(y))))
    assert bool((on[3][on[6]] == 0).all())


def test_graphs_one_capture_for_every_map(model):
    """SynthGraphs on prosody_a's inputs: three p_control maps (the fixture's, reversed along L, a
    constant 1.1) replay the first call's graphs -- where three scalar values capture anew --, and
    every call equals the eager forward with the same maps."""
    from fs2amd.graphs import SynthGraphs

    args, p_map, d_map, _, _ = load_prosody("prosody_a")
    model.set_precision("fp32")
    a = _dev(args)
    P, D = p_map.to(DEV), d_map.to(DEV)
    assert float(P.max()) <= 2.0
    synth = SynthGraphs(model)
    with torch.no_grad():
        _same(synth(**a, p_control=P, d_control=D), model(**a, p_control=P, d_control=D))
        first = synth.captures
        assert first >= 2
        for pm in (P.flip(1), torch.full_like(P, 1.1)):
            _same(synth(**a, p_control=pm, d_control=D), model(**a, p_control=pm, d_control=D))
            assert synth.captures == first
        # a broadcastable map uses the same graph (the marker, not the shape, is in the key)
        _same(synth(**a, p_control=P[:, :1], d_control=D), model(**a, p_control=P[:, :1], d_control=D))
        assert synth.captures == first
        # another duration map: same stage-1 graph; stage 2 may capture for a new T bucket
        D2 = D.flip(1).contiguous()
        _same(synth(**a, p_control=P, d_control=D2), model(**a, p_control=P, d_control=D2))
        assert len(synth._g1) == 1
        # the contrast (today's behaviour): every new scalar value is a new stage-1 capture
        n = synth.captures
        for i, pc in enumerate((0.9, 1.0, 1.1)):
            _same(synth(**a, p_control=pc, d_control=D), model(**a, p_control=pc, d_control=D))
            assert synth.captures > n
            n = synth.captures
        assert len(synth._g1) == 4
    synth.close()


def test_map_errors_through_forward(model):
    args, p_map, d_map, _, _ = load_prosody("prosody_b")
    model.set_precision("fp32")
    a = _dev(args)
    B, L = a["texts"].shape
    with torch.no_grad():
        with pytest.raises((ValueError, RuntimeError), match="HIP"):
            model(**a, p_control=p_map)  # a CPU map
        with pytest.raises((ValueError, RuntimeError), match="broadcast"):
            model(**a, d_control=torch.ones(B, L + 1, device=DEV))
        with pytest.raises((ValueError, RuntimeError), match="float"):
            model(**a, p_control=torch.ones(B, L, device=DEV, dtype=torch.int64))
        va = model.variance_adaptor
        try:
            va.pitch_feature_level = "frame_level"
            with pytest.raises(ValueError, match="frame_level"):
                model(**a, p_control=p_map.to(DEV))
        finally:
            va.pitch_feature_level = "phoneme_level"
    torch.cuda.synchronize()
