"""Mixture / curve conditioning on the GPU (include/fs2hip_cond_mix.h).

1-3  ops.cond_mix / ops.cond_mix_rows: one-hot weights give the bits of ops.cond_vectors; general
     weights stay within 2^-17 * S of the float64 restatement tests/_condmix.py, S = sum_k |W[n, k]|
     |cat[k]| + |b[n]| (64 chained fmaf, three adds, the bias and at most five mixing fmaf are 73
     roundings of 2^-24 each, under 128 = 2^-17 / 2^-24); a row's bits do not depend on its batch.
     The in-place add of the rows kernel is one more rounding of that size on |x| + emo, so its
     bound is the same with S + |x| (74 roundings), plus the bf16 rounding for bf16 x: half a unit in
     the last of its 8 significant bits, 2^-8 |y|.
4-6  FastSpeech2.forward: one-hot weights equal the id call bit for bit, the fixtures condmix_a /
     condmix_b meet test_gpu_model.py's fp32 bounds against the reference, a constant curve equals
     the utterance mixture (fp32, all ten outputs), and in bf16 stays within
     test_targets_bf16_vs_reference's bound.
7    SynthGraphs: weights are graph inputs (one stage-1 graph per form serves every value).
8    the ValueErrors.
"""
import numpy as np
import pytest
import torch

import _condmix as CM
from _common import OUT_NAMES, configs, load_case, oracle_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -7.25
U17 = 2.0 ** -17
NAMES = ("speakers", "emotions", "arousals", "valences")
KEYS = ("spk_table", "emo_table", "aro_table", "val_table", "lin_w", "lin_b")


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd.model import FastSpeech2

    pc, mc, _ = configs()
    m = FastSpeech2(pc, mc)
    m.load_state_dict(oracle_state_dict())
    return m.to(DEV).eval()


class Params:
    """The conditioning parameters on the host (numpy, for _condmix) and on the device."""

    def __init__(self, tensors):
        self.np = {k: v.numpy() for k, v in zip(KEYS, tensors)}
        self.dev = {k: v.to(DEV).contiguous() for k, v in zip(KEYS, tensors)}
        self.D = tensors[4].shape[0]
        self.n = {"speakers": tensors[0].shape[0], "emotions": tensors[1].shape[0], "arousals": tensors[2].shape[0],
                  "valences": tensors[3].shape[0]}

    def args(self, spk, emo, aro, val, speaker=True, emotion=True):
        d = self.dev
        return (spk if speaker else None, d["spk_table"] if speaker else None, emo, aro, val,
                d["emo_table"] if emotion else None, d["aro_table"], d["val_table"], d["lin_w"], d["lin_b"], self.D)

    def rows_args(self, emo, aro, val):
        d = self.dev
        return (emo, aro, val, d["emo_table"], d["aro_table"], d["val_table"], d["lin_w"], d["lin_b"])


@pytest.fixture(scope="module")
def p256():
    """D = 256 with the synthetic model's tables (10 speakers; 5 / 4 / 5 rows of width 128 / 64 / 64)."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    sd = oracle_state_dict()
    return Params([sd[k].float() for k in ("speaker_emb.weight", "emotion_emb.weight", "arousal_emb.weight",
                                            "valence_emb.weight", "emotion_linear.0.weight", "emotion_linear.0.bias")])


@pytest.fixture(scope="module")
def p72():
    """D = 72, widths 36 / 18 / 18: (d_emo + d_aro + d_val) % 16 != 0, the scalar path; D % 64 != 0."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    return Params([r(7, 72), r(5, 36), r(3, 18), r(6, 18), r(72, 72) / 8, r(72)])


def _ids(P, B, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randint(0, P.n[k], (B,), generator=g) for k in NAMES}


def _hot(ids, n):
    return torch.nn.functional.one_hot(ids, n).float()


def _weights(P, shape, seed):
    """Random weights used as given: signs mixed, sums anywhere in about [-1, 2]."""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(*shape, P.n[k], generator=g) - 0.25) * (2.0 / P.n[k]) for k in NAMES}


def _dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


# ---- 1. ops, one-hot ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 8, 9, 17])
@pytest.mark.parametrize("speaker,emotion", [(True, True), (False, True), (True, False)])
def test_cond_mix_one_hot_equals_cond_vectors(p256, B, speaker, emotion):
    _one_hot_case(p256, B, speaker, emotion)


def test_cond_mix_one_hot_equals_cond_vectors_scalar_path(p72):
    _one_hot_case(p72, 9, True, True)


def _one_hot_case(P, B, speaker, emotion):
    from fs2amd import ops

    ids = _dev(_ids(P, B, 10 + B))
    hot = {k: _hot(ids[k], P.n[k]) for k in NAMES}
    ref = ops.cond_vectors(*P.args(*[ids[k] for k in NAMES], speaker=speaker, emotion=emotion))
    got = ops.cond_mix(*P.args(*[hot[k] for k in NAMES], speaker=speaker, emotion=emotion))
    byid = ops.cond_mix(*P.args(*[ids[k] for k in NAMES], speaker=speaker, emotion=emotion))
    torch.cuda.synchronize()
    for r, g, i, on in zip(ref, got, byid, (speaker, emotion)):
        if not on:
            assert r is None and g is None and i is None
            continue
        assert g.dtype == torch.float32 and g.shape == (B, P.D)
        assert torch.equal(g, r) and torch.equal(i, r)


# ---- 2. ops, general weights -------------------------------------------------------------------------
class Guarded:
    """A contiguous f32 tensor of ``shape`` with GUARD sentinel words before and behind it."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        self.view, self.n = self.buf[GUARD:GUARD + n].view(*shape), n

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all())


@pytest.mark.parametrize("which", ["p256", "p72"])
@pytest.mark.parametrize("kinds", ["wwww", "iwiw", "wiwi"])
def test_cond_mix_general_weights_within_bound(request, which, kinds):
    from fs2amd import ops

    P = request.getfixturevalue(which)
    B = 9
    ids, w = _ids(P, B, 3), _weights(P, (B,), 4)
    inp = {k: (w[k] if c == "w" else ids[k]) for k, c in zip(NAMES, kinds)}
    so, eo = Guarded((B, P.D)), Guarded((B, P.D))
    d = _dev(inp)
    ops.cond_mix(*P.args(*[d[k] for k in NAMES]), spk_out=so.view, emo_out=eo.view)
    torch.cuda.synchronize()
    assert so.intact() and eo.intact()
    host = {k: v.numpy() for k, v in inp.items()}
    spk, s_spk = CM.speaker_vectors(P.np["spk_table"], host["speakers"])
    emo, s_emo = CM.emotion_vectors(P.np, host["emotions"], host["arousals"], host["valences"])
    for name, got, ref, S in (("spk", so.view, spk, s_spk), ("emo", eo.view, emo, s_emo)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        print(f"{which} {kinds} {name}: max err / (2^-17 S) = {(err / (U17 * S + 1e-300)).max():.3f}")
        assert (err <= U17 * S).all(), (name, float((err / (U17 * S + 1e-300)).max()))
    assert (emo > 0).any() and (emo == 0).any()  # both sides of the ReLU


# ---- 3. ops, rows ------------------------------------------------------------------------------------
def _x(B, L, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, D, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (9, 17)])
def test_rows_with_constant_weights_equal_the_utterance_vector(p256, B, L, dtype):
    from fs2amd import ops

    P = p256
    w = _dev(_weights(P, (B,), 20 + B))
    ids = _dev(_ids(P, B, 21))
    x0 = _x(B, L, P.D, dtype, 22).to(DEV)
    for emo, aro, val in ((w["emotions"], w["arousals"], w["valences"]), (w["emotions"], ids["arousals"], w["valences"])):
        _, vec = ops.cond_mix(*P.args(None, emo, aro, val, speaker=False))
        want = (x0.float() + vec[:, None, :]).to(dtype)
        # every position's weights equal to the utterance row, as [B, L, n] rows ...
        rep = lambda t: t[:, None, :].expand(-1, L, -1).contiguous() if t.is_floating_point() else t
        got = ops.cond_mix_rows(x0.clone(), rep(emo), rep(aro), rep(val), *P.rows_args(None, None, None)[3:])
        assert got.dtype == dtype and torch.equal(got, want)
        # ... and broadcast by the kernel from [B, n]; one curve among them is enough
        got = ops.cond_mix_rows(x0.clone(), rep(emo), aro, val, *P.rows_args(None, None, None)[3:])
        assert torch.equal(got, want)


@pytest.mark.parametrize("which", ["p256", "p72"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (9, 17)])
def test_rows_with_per_position_weights_within_bound(request, which, B, L, dtype):
    from fs2amd import ops

    P = request.getfixturevalue(which)
    w = _weights(P, (B, L), 30 + L)
    ids = _ids(P, B, 31)
    mix = _weights(P, (B,), 32)
    inp = {"emotions": w["emotions"], "arousals": mix["arousals"], "valences": w["valences"]}
    if B == 3:
        inp["valences"] = ids["valences"]
    x0 = _x(B, L, P.D, dtype, 33)
    buf = torch.full((B * L * P.D + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    x = buf[GUARD:GUARD + B * L * P.D].view(B, L, P.D)
    x.copy_(x0)
    d = _dev(inp)
    got = ops.cond_mix_rows(x, d["emotions"], d["arousals"], d["valences"], *P.rows_args(None, None, None)[3:])
    torch.cuda.synchronize()
    assert got.data_ptr() == x.data_ptr()
    b = buf.float().cpu()
    assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all()
    emo, S = CM.emotion_vectors(P.np, *[inp[k].numpy() for k in NAMES[1:]], L=L)
    ref = CM.add(x0.float().numpy(), emo=emo)
    bound = U17 * (S + np.abs(x0.float().numpy().astype(np.float64)))
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)  # bf16: 8 significant bits, RNE
    err = np.abs(got.float().cpu().numpy().astype(np.float64) - ref)
    print(f"{which} rows {B}x{L} {dtype}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_rows_alone_equal_rows_inside_a_larger_batch(p256, dtype):
    from fs2amd import ops

    P, B, L = p256, 9, 17
    w = _dev(_weights(P, (B, L), 40))
    x0 = _x(B, L, P.D, dtype, 41).to(DEV)
    tabs = P.rows_args(None, None, None)[3:]
    big = ops.cond_mix_rows(x0.clone(), w["emotions"], w["arousals"], w["valences"], *tabs)
    for b in (0, 4, 8):  # an utterance alone: another B, another slot in the 16-row tiles
        one = ops.cond_mix_rows(x0[b:b + 1].clone(), *[w[k][b:b + 1].contiguous() for k in NAMES[1:]], *tabs)
        assert torch.equal(one[0], big[b]), b
    # one position alone (L = 1), against the utterance-level kernel too
    b, i = 5, 11
    row = [w[k][b:b + 1, i].contiguous() for k in NAMES[1:]]
    one = ops.cond_mix_rows(x0[b:b + 1, i:i + 1].clone(), *[r[:, None, :].contiguous() for r in row], *tabs)
    assert torch.equal(one[0, 0], big[b, i])
    _, vec = ops.cond_mix(*P.args(None, *row, speaker=False))
    assert torch.equal((x0[b, i].float() + vec[0]).to(dtype), big[b, i])


# ---- 4. model, one-hot equals ids ----------------------------------------------------------------------
def _run(model, args, controls, prec, **over):
    from fs2amd.data import to_device

    model.set_precision(prec)
    p_c, e_c, d_c = controls
    a = to_device(args, DEV)
    a.update({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in over.items()})
    with torch.no_grad():
        out = model(**a, p_control=p_c, e_control=e_c, d_control=d_c)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    assert len(a) == len(b) == 10
    for name, x, y in zip(OUT_NAMES, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), name


N_MODEL = {"speakers": 10, "emotions": 5, "arousals": 4, "valences": 5}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["mini_free_ctrl", "cfg2_free"])
def test_model_one_hot_equals_ids(model, case, prec):
    args, controls, _, _ = load_case(case)
    ref = _run(model, args, controls, prec)
    got = _run(model, args, controls, prec, **{k: _hot(args[k], N_MODEL[k]) for k in NAMES})
    _same(got, ref)


# ---- 5. model against the reference --------------------------------------------------------------------
def _fixture_weights(z):
    return {k: torch.from_numpy(z["w_" + k]) for k in NAMES}


@pytest.mark.parametrize("case", ["condmix_a", "condmix_b"])
def test_model_fp32_matches_reference(model, case):
    args, controls, outs, z = load_case(case)
    got = _run(model, args, controls, "fp32", **_fixture_weights(z))
    for name, g in zip(OUT_NAMES, got):
        ref, g = outs[name], g.detach().cpu().numpy()
        assert g.shape == ref.shape, (name, g.shape, ref.shape)
        if name in ("mel", "postnet_mel", "p_pred", "e_pred", "log_d"):
            err = float(np.abs(g - ref).max())
            print(f"{case} {name}: max err {err:.3e}")
            assert err <= (2e-3 if "mel" in name else 5e-4), (name, err)
        else:
            np.testing.assert_array_equal(g.astype(ref.dtype), ref, err_msg=name)


# ---- 6. model, a curve that is constant -----------------------------------------------------------------
@pytest.mark.parametrize("case", ["condmix_a", "condmix_b"])
def test_model_constant_curve_equals_mixture_fp32(model, case):
    args, controls, _, z = load_case(case)
    w = _fixture_weights(z)
    L = args["max_src_len"]
    if w["emotions"].dim() == 3:  # condmix_b: the row of phoneme 0 everywhere
        w["emotions"] = w["emotions"][:, 0].contiguous()
    ref = _run(model, args, controls, "fp32", **w)
    rep = lambda t: t[:, None, :].expand(-1, L, -1).contiguous()
    _same(_run(model, args, controls, "fp32", **dict(w, emotions=rep(w["emotions"]))), ref)
    _same(_run(model, args, controls, "fp32", **dict(w, arousals=rep(w["arousals"]))), ref)


def _valid_err(got_post, ref_post, ml):
    valid = (np.arange(ref_post.shape[1])[None, :] < ml[:, None])[..., None]
    e = np.abs(got_post - ref_post) * valid
    return float(e.max()), float(e.sum() / (valid.sum() * ref_post.shape[2]))


def test_model_constant_one_hot_curve_bf16_within_the_id_paths_bound(model):
    """The teacher-forced cfg2 fixture of test_gpu_model.py::test_targets_bf16_vs_reference with
    one-hot constant curves equal to its ids: the curve path rounds the encoder output to bf16
    once more than the id path (after the speaker add, then after the emotion add) and must stay
    within that test's bound (head max 0.075, mean 0.0125; checksums 4e-3) against the reference."""
    args, controls, outs, z = load_case("cfg2_targets")
    L, head = args["max_src_len"], 4
    curves = {k: _hot(args[k], N_MODEL[k])[:, None, :].expand(-1, L, -1).contiguous() for k in NAMES[1:]}
    for what, over in (("ids", {}), ("curves", curves)):
        got = _run(model, args, controls, "bf16", **over)
        ml = got[9].cpu().numpy()
        np.testing.assert_array_equal(ml, outs["mel_lens_out"])
        mx, mean = _valid_err(got[1][:head].float().cpu().numpy(), outs["postnet_mel_head"], ml[:head])
        post = got[1].double().cpu()
        valid = (torch.arange(post.shape[1])[None, :] < got[9].cpu()[:, None]).double()[..., None]
        ck_abs, ck_sum = (post.abs() * valid).sum((1, 2)).numpy(), (post * valid).sum((1, 2)).numpy()
        rel_abs = np.abs(ck_abs - z["ck_post_valid_abs"]) / z["ck_post_valid_abs"]
        sum_err = np.abs(ck_sum - z["ck_post_valid_sum"]) / (ml.astype(np.float64) * 80)
        print(f"cfg2_targets bf16 {what}: head max {mx:.4f} mean {mean:.5f}; |post| checksum rel max "
              f"{rel_abs.max():.2e}; per-frame-value sum error max {sum_err.max():.2e}")
        assert mx <= 0.075 and mean <= 0.0125, (what, mx, mean)
        assert rel_abs.max() <= 4e-3 and sum_err.max() <= 4e-3, (what, rel_abs.max(), sum_err.max())


# ---- 7. SynthGraphs --------------------------------------------------------------------------------------
def test_synth_graphs_take_weights_as_inputs(model):
    from fs2amd.data import to_device
    from fs2amd.graphs import SynthGraphs

    model.set_precision("fp32")
    args, _, _, z = load_case("condmix_a")
    b = to_device({k: v for k, v in args.items() if k not in ("mels", "mel_lens", "max_mel_len", "d_targets")}, DEV)
    L = b["max_src_len"]
    w1 = {k: v.to(DEV) for k, v in _fixture_weights(z).items()}
    # other values; the second of each pair close enough to the first to stay in its decoder buckets
    w2 = {k: (0.999 * v + 0.001 * v.flip(0)).contiguous() for k, v in w1.items()}
    w3 = {k: v.flip(0).contiguous() for k, v in w1.items()}
    rep = lambda t: t[:, None, :].expand(-1, L, -1).contiguous()
    ramp = torch.linspace(0, 1, L, device=DEV)[None, :, None]
    curve = lambda w: dict(b, **dict(w, emotions=(rep(w["emotions"]) * (1 - ramp) +
                                                 rep(w["emotions"].flip(0)) * ramp).contiguous()))
    synth = SynthGraphs(model)
    with torch.no_grad():
        _same(synth(**b), model(**b))
        n1 = len(synth._g1)
        c0 = synth.captures
        _same(synth(**dict(b, **w1)), model(**dict(b, **w1)))
        c1 = synth.captures
        assert c1 > c0 and len(synth._g1) == n1 + 1
        _same(synth(**dict(b, **w2)), model(**dict(b, **w2)))
        assert synth.captures == c1                        # the same graphs, other weights
        _same(synth(**dict(b, **w3)), model(**dict(b, **w3)))
        assert len(synth._g1) == n1 + 1                    # one stage-1 graph for every mixture
        c1 = synth.captures
        _same(synth(**curve(w1)), model(**curve(w1)))
        c2 = synth.captures
        assert c2 > c1 and len(synth._g1) == n1 + 2
        _same(synth(**curve(w2)), model(**curve(w2)))
        assert synth.captures == c2
        _same(synth(**curve(w3)), model(**curve(w3)))
        assert len(synth._g1) == n1 + 2
        c2 = synth.captures
        _same(synth(**b), model(**b))                      # the id call still has its own graph
        assert synth.captures == c2 and len(synth._g1) == n1 + 2
    synth.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------
def test_value_errors_on_the_device(model):
    from fs2amd.data import to_device

    model.set_precision("fp32")
    args, _, _, z = load_case("condmix_a")
    b = to_device(args, DEV)
    B, L = b["texts"].shape
    ones = lambda *s: torch.ones(*s, device=DEV)
    bad = [dict(emotions=ones(B, 4)), dict(arousals=ones(B, L + 1, 4)), dict(valences=ones(B, L, 4)),
           dict(speakers=ones(B, L, 10)), dict(emotions=torch.ones(B, 5)), dict(arousals=ones(B)),
           dict(valences=ones(B, L, 5, 1)), dict(speakers=ones(B + 1, 10))]
    for over in bad:
        with pytest.raises(ValueError):
            with torch.no_grad():
                model(**dict(b, **over))
    from fs2amd.graphs import SynthGraphs

    synth = SynthGraphs(model)
    sb = {k: v for k, v in b.items() if k not in ("mels", "mel_lens", "max_mel_len", "d_targets")}
    for over in bad[:5]:
        with pytest.raises(ValueError):
            with torch.no_grad():
                synth(**dict(sb, **over))
    assert synth.captures == 0
    model.train()
    try:
        with pytest.raises(ValueError, match="training"):
            model(**dict(b, emotions=ones(B, 5)))
    finally:
        model.eval()
