"""fs2_enc_attn_block's row-split form (enc_attn_rows_kernel: four workgroups per utterance, each
with K / V of the whole utterance, Q, attention, fc and LayerNorm of its own 16 query rows) against
the one-workgroup form it replaces (FS2_ENC_ROWS=0).

Every accumulator keeps the one-workgroup form's k order and the LayerNorm its partial grouping, so
the two are compared with torch.equal; the float64 bounds are those of test_gpu_enc_block.py. The
switch is read at every launch. L = 17 leaves quarter 1 with one row and quarters 2-3 empty; B is
not always a multiple of 8; lengths 0 / 1 / 15 / 16 / 17 / L put the valid / padded boundary on,
beside and inside a quarter.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(64, 64), (7, 64), (5, 37), (9, 17), (2, 16), (4, 48), (3, 1)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops, _lib as L

    return ops, L


def _weights(g, D=256):
    wqkv = torch.randn(3 * D, D, device=DEV, generator=g) / D ** 0.5
    bqkv = 0.1 * torch.randn(3 * D, device=DEV, generator=g)
    wfc = torch.randn(D, D, device=DEV, generator=g) / D ** 0.5
    bfc = 0.1 * torch.randn(D, device=DEV, generator=g)
    gam = 1 + 0.1 * torch.randn(D, device=DEV, generator=g)
    bet = 0.1 * torch.randn(D, device=DEV, generator=g)
    return wqkv, bqkv, wfc, bfc, gam, bet


def _lens(B, L, seed):
    """Random lengths with L, 0, 1, 15, 16, 17 forced in (those that fit L, while the batch has room)."""
    lens = torch.randint(0, L + 1, (B,), generator=torch.Generator().manual_seed(seed))
    forced = [L] + [v for v in (0, 1, 15, 16, 17) if v < L]
    for i, v in enumerate(forced[:B]):
        lens[i] = v
    return lens.to(DEV)


def _ref64(x, lens, wqkv, bqkv, wfc, bfc, gam, bet, eps=1e-5, H=2, dk=128):
    """float64 statement of the sub-layer on the bf16-rounded weights / input."""
    xd = x.double()
    B, L, D = x.shape
    qkv = xd @ wqkv.to(torch.bfloat16).double().t() + bqkv.double()
    q, k, v = qkv.split(D, -1)
    heads = lambda t: t.view(B, L, H, dk).transpose(1, 2)
    s = heads(q) @ heads(k).transpose(-1, -2) / dk ** 0.5
    keymask = torch.arange(L, device=DEV)[None, :] >= lens[:, None]
    s = s.masked_fill(keymask[:, None, None, :], float("-inf"))
    a = torch.softmax(s, -1).nan_to_num(0.0)
    o = (a @ heads(v)).transpose(1, 2).reshape(B, L, D)
    y = o @ wfc.to(torch.bfloat16).double().t() + bfc.double() + xd
    y = torch.nn.functional.layer_norm(y, (D,), gam.double(), bet.double(), eps)
    return y.masked_fill(keymask[..., None], 0.0)


@pytest.mark.parametrize("B,L", SHAPES)
def test_rows_form_equals_one_workgroup_and_float64(gpu, monkeypatch, B, L):
    ops, _ = gpu
    seed = 10 * B + L
    g = torch.Generator(device=DEV).manual_seed(seed)
    wqkv, bqkv, wfc, bfc, gam, bet = _weights(g)
    x = torch.randn(B, L, 256, device=DEV, generator=g).to(torch.bfloat16)
    lens = _lens(B, L, seed)
    ln = (gam, bet, 1e-5)
    wq, wf = ops.pack_frag_rows(wqkv), ops.pack_frag_rows(wfc)
    run = lambda: ops.enc_attn_block(x, lens, wq, bqkv, wf, bfc, ln, 2, 128, 128 ** 0.5)
    monkeypatch.setenv("FS2_ENC_ROWS", "0")
    one = run()
    monkeypatch.setenv("FS2_ENC_ROWS", "1")
    rows = run()
    again = run()
    torch.cuda.synchronize()
    assert torch.equal(rows, one), float((rows.float() - one.float()).abs().max())
    assert torch.equal(again, rows)
    pad = torch.arange(L, device=DEV)[None, :] >= lens[:, None]
    assert bool((rows[pad] == 0).all()), "padded rows must be zero"
    err = (rows.double() - _ref64(x, lens, wqkv, bqkv, wfc, bfc, gam, bet)).abs()
    print(f"rows form vs float64: max {float(err.max()):.4f} mean {float(err.mean()):.2e}")
    assert float(err.max()) <= 0.06 and float(err.mean()) <= 4e-3, (float(err.max()), float(err.mean()))


@pytest.mark.parametrize("B,L", SHAPES)
def test_rows_form_embed_equals_one_workgroup(gpu, monkeypatch, B, L):
    """EMBED form (x = bf16(emb[tok] + pe) built in the launch, both masks written by it): output and
    masks equal the one-workgroup form's; one out-of-vocabulary id gives a NaN row and raises the
    bad-id counter by exactly 1 (each of the utterance's four workgroups builds that row)."""
    ops, _ = gpu
    seed = 10 * B + L + 1
    g = torch.Generator(device=DEV).manual_seed(seed)
    wqkv, bqkv, wfc, bfc, gam, bet = _weights(g)
    vocab, T_mel = 50, 77
    table = torch.randn(vocab, 256, device=DEV, generator=g)
    pe = torch.randn(L + 3, 256, device=DEV, generator=g)
    tok = torch.randint(0, vocab, (B, L), device=DEV, generator=g)
    lens = _lens(B, L, seed)
    mel_lens = torch.randint(-2, 90, (B,), generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    ln = (gam, bet, 1e-5)
    wq, wf = ops.pack_frag_rows(wqkv), ops.pack_frag_rows(wfc)

    def run(form, tokens):
        monkeypatch.setenv("FS2_ENC_ROWS", form)
        sm = torch.zeros(B, L, device=DEV, dtype=torch.bool)
        mm = torch.zeros(B, T_mel, device=DEV, dtype=torch.bool)
        out = ops.enc_attn_block(None, lens, wq, bqkv, wf, bfc, ln, 2, 128, 128 ** 0.5, embed=(tokens, table, pe),
                                 masks=(sm, mel_lens, mm))
        torch.cuda.synchronize()
        return out, sm, mm

    one, sm0, mm0 = run("0", tok)
    rows, sm1, mm1 = run("1", tok)
    assert torch.equal(rows, one), float((rows.float() - one.float()).abs().max())
    assert torch.equal(sm1, sm0) and torch.equal(mm1, mm0)
    assert torch.equal(sm1, ops.length_mask(lens, L)) and torch.equal(mm1, ops.length_mask(mel_lens, T_mel))

    bad = ops.bad_id_counter(torch.device(DEV))
    bad.zero_()
    tok2 = tok.clone()
    tok2[0, L - 1] = vocab + 3  # utterance 0 has length L: a valid row, in the last non-empty quarter
    out, _, _ = run("1", tok2)
    count = int(bad.item())
    bad.zero_()
    assert count == 1, count
    assert bool(torch.isnan(out[0, L - 1].float()).all())
    assert not bool(torch.isnan(out[1:].float()).any())
    assert torch.equal(out[1:], one[1:])
