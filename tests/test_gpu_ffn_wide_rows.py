"""fs2_ffn_wide's second launch on whole rows (ffn_out_rows_kernel: a workgroup owns 16 or 32 rows x
all 256 output columns, so the LayerNorm needs no hand-off between workgroups) against the quarter
form it replaces (FS2_WIDE_OUT=0: 64-row x 64-column tiles, f32 pre-norm rows through the split-K
workspace, the last of 4 arrivers normalises).

The rows form keeps the quarter form's k order per wave, sums the 4 wave partials in wave order,
adds b2 and x in the same order and runs the same LayerNorm code on the same lane mapping, so the
two are compared with torch.equal; the float64 bounds are those of
test_gpu_ffn.py::test_ffn_wide_matches_float64_and_fused. Both switches are read at every launch.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(64, 64, 1024, 9), (8, 130, 1024, 9), (3, 37, 1024, 9), (1, 300, 1024, 9), (5, 50, 512, 3)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops, _lib as L

    return ops, L


def _weights(ops, F, ks, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w1 = torch.randn(F, 256, ks, device=DEV, generator=g) / (256 * ks) ** 0.5
    w2 = torch.randn(256, F, 1, device=DEV, generator=g) / F ** 0.5
    b1 = 0.1 * torch.randn(F, device=DEV, generator=g)
    b2 = 0.1 * torch.randn(256, device=DEV, generator=g)
    ln = (1 + 0.1 * torch.randn(256, device=DEV, generator=g), 0.1 * torch.randn(256, device=DEV, generator=g), 1e-5)
    return dict(w1=w1, w2=w2, b1=b1, b2=b2, ln=ln, w12=ops.pack_ffn_weights(w1, w2), ks=ks)


def _ref(x, lens, W, addvecs=()):
    """float64 statement on the same bf16 operands: per-sequence conv, the hidden rounded to bf16 where
    it is stored, LN(f w2^T + b2 + x), rows t >= len -> 0, + addvecs."""
    ks = W["ks"]
    xd = x.double()
    w1 = W["w1"].to(torch.bfloat16).double()
    w2 = W["w2"].to(torch.bfloat16).double()[:, :, 0]
    f = torch.nn.functional.conv1d(xd.transpose(1, 2), w1, W["b1"].double(), padding=(ks - 1) // 2).transpose(1, 2)
    f = torch.relu(f).to(torch.bfloat16).double()
    g, b, eps = W["ln"]
    y = torch.nn.functional.layer_norm(f @ w2.t() + W["b2"].double() + xd, (256,), g.double(), b.double(), eps)
    y = y * (torch.arange(x.shape[1], device=DEV)[None, :, None] < lens[:, None, None])
    for v in addvecs:
        y = y + v.double()[:, None, :]
    return y


def _case(B, T, seed):
    """Ragged lengths with T, 1, 3 and 0 forced in where the batch has room; x zero past each length."""
    lens_l = np.random.default_rng(seed).integers(0, T + 1, B).tolist()
    lens_l[0] = T
    if B > 2:
        lens_l[1], lens_l[2] = 1, 3
    if B > 3:
        lens_l[3] = 0
    lens = torch.tensor(lens_l, dtype=torch.int64, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    valid = (torch.arange(T, device=DEV)[None, :] < lens[:, None])[..., None]
    return lens, (torch.randn(B, T, 256, device=DEV, generator=g) * valid).to(torch.bfloat16)


def _run(monkeypatch, ops, form, rb, x, W, **kw):
    """One fs2_ffn_wide call with FS2_WIDE_OUT = form and FS2_WIDE_OUT_RB = rb (None: unset)."""
    monkeypatch.setenv("FS2_WIDE_OUT", form)
    if rb is None:
        monkeypatch.delenv("FS2_WIDE_OUT_RB", raising=False)
    else:
        monkeypatch.setenv("FS2_WIDE_OUT_RB", rb)
    y = ops.ffn_wide(x, W["w12"], W["b1"], W["b2"], ks=W["ks"], pad=(W["ks"] - 1) // 2, ln=W["ln"], **kw)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("B,T,F,ks", SHAPES)
def test_rows_form_equals_quarter_form_and_float64(gpu, monkeypatch, B, T, F, ks):
    """FS2_WIDE_OUT=1 (the form rule's choice), both forced RB instances and a repeated launch are
    bit-identical to FS2_WIDE_OUT=0; against float64 within max 3e-2 / mean 2e-3. 3 x 37 = 111 rows
    is no multiple of 16; 1 x 300 ends inside a 32-row tile."""
    ops, _ = gpu
    seed = 100 + B
    W = _weights(ops, F, ks, seed)
    lens, x = _case(B, T, seed)
    quarter = _run(monkeypatch, ops, "0", None, x, W, lens=lens)
    rows = _run(monkeypatch, ops, "1", None, x, W, lens=lens)
    assert torch.equal(rows, quarter)
    assert torch.equal(_run(monkeypatch, ops, "1", None, x, W, lens=lens), rows)
    for rb in ("1", "2"):
        assert torch.equal(_run(monkeypatch, ops, "1", rb, x, W, lens=lens), quarter), rb
    err = (rows.double() - _ref(x, lens, W)).abs()
    print(f"rows form vs float64: max {float(err.max()):.4f} mean {float(err.mean()):.2e}")
    assert float(err.max()) <= 3e-2 and float(err.mean()) <= 2e-3, (float(err.max()), float(err.mean()))


def test_rows_form_addvecs_and_packed(gpu, monkeypatch):
    """Speaker / emotion vectors (after the mask, every row) and packed rows of a SeqLayout sized for
    fewer rows than its capacity (rows_hint): each bit-identical to the quarter form at both RB, and
    packed == padded."""
    ops, _ = gpu
    W = _weights(ops, 1024, 9, 61)
    B, T = 6, 70
    lens = torch.tensor([70, 0, 1, 33, 69, 12], dtype=torch.int64, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(62)
    valid = (torch.arange(T, device=DEV)[None, :] < lens[:, None])[..., None]
    x = (torch.randn(B, T, 256, device=DEV, generator=g) * valid).to(torch.bfloat16)
    v1, v2 = (torch.randn(B, 256, device=DEV, generator=g) for _ in range(2))
    kw = dict(lens=lens, addvec1=v1, addvec2=v2)
    quarter = _run(monkeypatch, ops, "0", None, x, W, **kw)
    for rb in (None, "1", "2"):
        assert torch.equal(_run(monkeypatch, ops, "1", rb, x, W, **kw), quarter), rb
    err = (quarter.double() - _ref(x, lens, W, (v1, v2))).abs()
    assert float(err.max()) <= 3e-2 and float(err.mean()) <= 2e-3, (float(err.max()), float(err.mean()))

    lay = ops.SeqLayout(lens, T)
    R = int(lay.cu[-1])
    lay.rows_hint = ops.rows_bucket(R, lay.capacity, 64)
    assert R < lay.rows_hint < lay.capacity
    rm = lay.rowmap.long()
    ok = rm >= 0
    xp = x.new_zeros(lay.capacity, 256)
    xp[rm[ok]] = x.reshape(-1, 256)[ok]
    padded = _run(monkeypatch, ops, "0", None, x, W, lens=lens).reshape(-1, 256)[ok]
    for form, rb in (("0", None), ("1", None), ("1", "1"), ("1", "2")):
        gp = _run(monkeypatch, ops, form, rb, xp, W, layout=lay)
        assert torch.equal(gp[:R], padded), (form, rb)
