"""fs2_pn_head3 — mel_linear and the PostNet's layers 0..2 in one launch — against the three
launches it replaces (fs2_conv1d KS = 1 with the bf16 out2 copy, fs2_wconv with w2, fs2_wconv):
BIT-EXACT f32 mel and bf16 layer-2 output. The fused kernel runs the same MFMA with the same
operands in the same k order per output element and rounds to bf16 at the same three places, so
there is no tolerance: every case asserts torch.equal.

Weights: the model's own packed PostNet / mel_linear weights from synth_weights.fill_module.
Shapes are the smallest that reach every path of the tile logic (108 owned rows per workgroup,
origin 108 i - 2, 120 / 116 / 112-row mel / y1 / y2 tiles):
* B = 3, T = 150 (450 rows, 5 workgroups): sequence ends at 150 and 300 fall inside tiles; the
  valid lengths put the first padded frame (row map -1) one row before and one row after a tile
  edge; padded frames must come out as the bias;
* B = 4, T = 109: sequence ends 1, 2 and 3 rows past a tile edge (109 / 218 / 327 vs 108 / 216 / 324);
* T = 3 and T = 5 (B = 4): sequences shorter than the combined halo, every tap mask in use;
* one sequence of 108, 109 and 217 rows: the last workgroup's edges;
* decoder rows of magnitude ~50: tanh saturates in all three layers;
* decoder rows given padded (no row map).
Packed PostNet rows (the valid-region form) stay on the three launches (runtime.pn_head3_ok), so
there is no packed case here.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from _common import configs
    from fs2amd import _lib as L, ops
    from fs2amd.model import FastSpeech2
    from fs2amd.synth_weights import fill_module

    pc, mc, _ = configs()
    model = fill_module(FastSpeech2(pc, mc), seed=0).to(DEV).eval()
    model.set_precision("bf16")
    return ops, L, model, model.packed(torch.device(DEV))


def _three(ops, L, P, x, B, T, lay):
    """Today's launches: mel_linear (+ its bf16 copy), layers 0 + 1, layer 2."""
    l0, l1, l2 = P.postnet[:3]
    mel_bf = torch.empty(B, T, 80, device=DEV, dtype=torch.bfloat16)
    mel = ops.conv1d(x, P.mel_w, P.mel_b, cin=256, ks=1, pad=0, compute=L.FS2_BF16, epilogue=L.EPI_BIAS,
                     out_dtype=L.FS2_F32, src_layout=lay, out2=mel_bf)
    y = ops.wconv(mel_bf, l0.wfr, l0.b, ks=5, pad=2, second=(l1.wfr, l1.b))
    return mel, mel_bf, ops.wconv(y, l2.wfr, l2.b, ks=5, pad=2)


def _one(ops, P, x, B, T, lay, mel_bf=None):
    return ops.pn_head3(x, P.mel_w, P.mel_b, [(l.wfr, l.b) for l in P.postnet[:3]], B, T, src_layout=lay,
                        mel_bf=mel_bf)


def _packed_case(ops, lens, T, seed, scale=1.0):
    lens = torch.tensor(lens, device=DEV, dtype=torch.int64)
    lay = ops.SeqLayout(lens, T)
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (scale * torch.randn(lay.capacity, 256, device=DEV, generator=g)).to(torch.bfloat16)
    return x, lay, lens


def _check(ops, L, P, x, B, T, lay):
    mel3, _, y3 = _three(ops, L, P, x, B, T, lay)
    mel1, y1 = _one(ops, P, x, B, T, lay)
    torch.cuda.synchronize()
    assert torch.equal(mel1, mel3), float((mel1 - mel3).abs().max())
    assert torch.equal(y1, y3), float((y1.float() - y3.float()).abs().max())
    return mel1, y1


def test_boundaries_inside_tiles_and_padded_frames(env):
    ops, L, model, P = env
    B, T = 3, 150
    # first padded frame at rows 107 (one before the edge 108) and 150 + 67 = 217 (one after 216)
    x, lay, lens = _packed_case(ops, [107, 67, 150], T, 1)
    mel3, mel_bf3, y3 = _three(ops, L, P, x, B, T, lay)
    mel_bf1 = torch.full((B, T, 80), 7.0, device=DEV, dtype=torch.bfloat16)
    mel1, y1 = _one(ops, P, x, B, T, lay, mel_bf=mel_bf1)
    torch.cuda.synchronize()
    assert torch.equal(mel1, mel3) and torch.equal(y1, y3)
    assert torch.equal(mel_bf1, mel_bf3)  # the optional bf16 copy: the rounding out2 does
    pad = torch.arange(T, device=DEV)[None, :] >= lens[:, None]
    assert int(pad.sum()) == 43 + 83
    assert torch.equal(mel1[pad], P.mel_b.float().expand(int(pad.sum()), 80))  # a padded frame gets the bias


@pytest.mark.parametrize("B,T,lens,seed", [
    (4, 109, [109, 50, 108, 1], 2),   # sequence ends just past the tile edges
    (4, 3, [3, 1, 2, 3], 3),          # shorter than the halo
    (4, 5, [5, 4, 1, 5], 4),
    (1, 108, [108], 5),               # exactly one workgroup
    (1, 109, [109], 6),               # one row into a second
    (1, 217, [217], 7),               # one row into a third
    (1, 217, [216], 8),               # ... that row a padded frame
])
def test_equals_three_launches(env, B, T, lens, seed):
    ops, L, model, P = env
    x, lay, _ = _packed_case(ops, lens, T, seed)
    _check(ops, L, P, x, B, T, lay)


def test_saturated_tanh(env):
    ops, L, model, P = env
    x, lay, _ = _packed_case(ops, [150, 97, 131], 150, 9, scale=50.0)
    mel, y = _check(ops, L, P, x, 3, 150, lay)
    assert bool(torch.isfinite(mel).all()) and bool(torch.isfinite(y.float()).all())


def test_padded_decoder_rows(env):
    """No row map: the decoder rows are the padded [B, T, 256] rows themselves."""
    ops, L, model, P = env
    g = torch.Generator(device=DEV).manual_seed(10)
    x = torch.randn(2, 113, 256, device=DEV, generator=g).to(torch.bfloat16)
    _check(ops, L, P, x, 2, 113, None)


def test_forward_switch_on_equals_off(env, monkeypatch):
    """The whole forward, eager, B = 2: all ten outputs bit-identical with FS2_PN_HEAD3 on and off,
    and the fused launch is what ran with it on."""
    ops, L, model, P = env
    from fs2amd.data import synth_batch, to_device

    args = to_device(synth_batch(2, 12, 20, seed=11), DEV)
    calls = []
    real = ops.pn_head3
    monkeypatch.setattr(ops, "pn_head3", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("FS2_PN_HEAD3", sw)
        n0 = len(calls)
        with torch.no_grad():
            outs[sw] = model(**args)
        torch.cuda.synchronize()
        assert (len(calls) - n0 > 0) == (sw == "1")
    assert len(outs["1"]) == len(outs["0"]) == 10
    for i, (a, b) in enumerate(zip(outs["1"], outs["0"])):
        assert torch.is_tensor(a) and torch.is_tensor(b), i
        assert a.dtype == b.dtype and torch.equal(a, b), i
