"""fs2_ffn, the eight-wave form of the packed unsplit 112-row PRE launch (two waves per SIMD, each
owning 32 weight rows of a quarter): bit-identical to the four-wave kernel (FS2_FFN_W8=0, read at
every launch), for the output rows and for the next block's Q|K|V rows.

* utterance boundaries inside a tile, tile boundaries inside utterances (halo rows recomputed on
  both sides), utterances shorter than the 4-row tap reach, a zero-length utterance, a 48-row last
  tile; a single partial tile; tiles exactly at utterance edges (every halo row masked);
* each with and without the Q|K|V epilogue; rows past the active rows are left untouched;
* a launch sized for more rows than the device row count (trailing workgroups exit);
* against the float64 statement of tests/test_gpu_ffn.py with its tolerance;
* repeated launches identical.
"""
import os

import pytest
import torch

from test_gpu_ffn import _pack, _ref, _weights, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [([37, 0, 130, 1, 64, 129, 130, 5], 130), ([3, 37], 37), ([112, 112], 112)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops, _lib as L

    return ops, L


@pytest.fixture(scope="module")
def params(gpu):
    """Seeded weights of the FFN (d_model 256, F 1024, k 9), the fc + LN1 prologue and a Q|K|V
    projection (nq 768): built once, never modified."""
    ops, L = gpu
    W = _weights(ops, L, seed=81)
    g = torch.Generator(device=DEV).manual_seed(82)
    wfc = torch.randn(256, 256, device=DEV, generator=g) / 16
    bfc = 0.1 * torch.randn(256, device=DEV, generator=g)
    ln1 = (1 + 0.1 * torch.randn(256, device=DEV, generator=g), 0.1 * torch.randn(256, device=DEV, generator=g), 1e-5)
    wq = torch.randn(768, 256, device=DEV, generator=g) / 16
    bq = 0.1 * torch.randn(768, device=DEV, generator=g)
    return dict(W=W, wfc=wfc, wfcf=ops.pack_frag_rows(wfc), bfc=bfc, ln1=ln1, wq=wq, wqf=ops.pack_frag_rows(wq), bq=bq)


class _form:
    """FS2_FFN_W8 for the launches inside: "0" = the four-wave kernel, None = the default."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("FS2_FFN_W8", None)
        if self.value is not None:
            os.environ["FS2_FFN_W8"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("FS2_FFN_W8", None)
        if self.old is not None:
            os.environ["FS2_FFN_W8"] = self.old


def _inputs(ops, lens_l, T, seed):
    lens = torch.tensor(lens_l, dtype=torch.int64, device=DEV)
    B = len(lens_l)
    x, att = _x(B, T, lens, seed), _x(B, T, lens, seed + 1)
    lay = ops.SeqLayout(lens, T)
    return lens, x, att, lay, _pack(lay, x), _pack(lay, att)


def _launch(ops, P, lay, xp, attp, qkv):
    """One 112-row unsplit PRE launch into sentinel-filled outputs: (out, qkv rows or None), whole
    capacity (the rows past the active ones must keep the sentinel)."""
    out = torch.full_like(xp, -3.0)
    r = ops.ffn(xp, P["W"]["w12"], P["W"]["b1"], P["W"]["b2"], ks=9, pad=4, ln=P["W"]["ln"], layout=lay, out=out,
                tile_rows=112, nsplit=1, pre=(attp, P["wfcf"], P["bfc"], P["ln1"]),
                next_qkv=(P["wqf"], P["bq"]) if qkv else None)
    torch.cuda.synchronize()
    return (r[0], r[1]) if qkv else (r, None)


def _both(ops, P, lay, xp, attp, qkv):
    with _form("0"):
        y4, q4 = _launch(ops, P, lay, xp, attp, qkv)
    with _form(None):
        y8, q8 = _launch(ops, P, lay, xp, attp, qkv)
    return y4, q4, y8, q8


@pytest.mark.parametrize("qkv", [False, True])
@pytest.mark.parametrize("lens_l,T", SHAPES)
def test_w8_equals_w4(gpu, params, lens_l, T, qkv):
    ops, _ = gpu
    _, _, _, lay, xp, attp = _inputs(ops, lens_l, T, 91)
    y4, q4, y8, q8 = _both(ops, params, lay, xp, attp, qkv)
    R = int(lay.cu[-1])
    assert R == sum(lens_l)
    assert torch.equal(y8, y4)  # whole capacity: the rows past R keep the sentinel in both
    assert bool((y8[R:] == -3.0).all()) and bool(torch.isfinite(y8[:R].float()).all())
    assert float(y8[:R].float().abs().max()) > 0.5  # (a launch that wrote nothing would also be "equal")
    if qkv:
        assert torch.equal(q8[:R], q4[:R])
        assert bool(torch.isfinite(q8[:R].float()).all())


def test_w8_rows_dev_below_launch_rows(gpu, params):
    """The launch is sized for 700 rows (7 tiles, rows_max below the capacity of 1040) and the device
    row count is 496: the workgroups of tiles 5 and 6 exit, the last active tile has 48 rows."""
    ops, _ = gpu
    lens_l, T = SHAPES[0]
    _, _, _, lay, xp, attp = _inputs(ops, lens_l, T, 92)
    lay.rows_hint = 700
    y4, q4, y8, q8 = _both(ops, params, lay, xp, attp, True)
    R = int(lay.cu[-1])
    assert R == 496
    assert torch.equal(y8, y4) and torch.equal(q8[:R], q4[:R])
    assert bool((y8[R:] == -3.0).all())
    del lay.rows_hint
    full, qfull = _launch(ops, params, lay, xp, attp, True)  # sized for the whole capacity: the same rows
    assert torch.equal(full, y8) and torch.equal(qfull[:R], q8[:R])


def test_w8_matches_float64(gpu, params):
    """The eight-wave form against the float64 statement (h = LN1(att wfc^T + bfc + x) rounded to bf16
    where the two-launch path stores it, then the FFN), tolerance of test_ffn_pre_fc_ln_prologue; the
    Q|K|V rows against float64 on the kernel's own output rows, tolerance of test_ffn_next_qkv_epilogue."""
    ops, _ = gpu
    P = params
    lens_l, T = SHAPES[0]
    lens, x, att, lay, xp, attp = _inputs(ops, lens_l, T, 93)
    with _form(None):
        y, qkv = _launch(ops, P, lay, xp, attp, True)
    R = int(lay.cu[-1])
    g1, b1n, eps1 = P["ln1"]
    h = torch.nn.functional.layer_norm(att.double() @ P["wfc"].to(torch.bfloat16).double().t() + P["bfc"].double() + x.double(),
                                       (256,), g1.double(), b1n.double(), eps1)
    valid = torch.arange(T, device=DEV)[None, :] < lens[:, None]
    h = (h * valid[..., None]).to(torch.bfloat16)
    refp = _ref(h, lens, P["W"]).reshape(-1, 256)[valid.reshape(-1)]
    err = (y[:R].double() - refp).abs()
    print(f"w8 vs float64: max {float(err.max()):.4f} mean {float(err.mean()):.2e}")
    assert float(err.max()) <= 0.1 and float(err.mean()) <= 6e-3, (float(err.max()), float(err.mean()))
    qref = y[:R].double() @ P["wq"].to(torch.bfloat16).double().t() + P["bq"].double()
    qerr = (qkv[:R].double() - qref).abs()
    scale = float(qref.abs().max())
    assert float(qerr.max()) <= 1e-2 * scale and float(qerr.mean()) <= 1e-3 * scale, (float(qerr.max()), scale)


def test_w8_repeat_launch_identical(gpu, params):
    ops, _ = gpu
    lens_l, T = SHAPES[0]
    _, _, _, lay, xp, attp = _inputs(ops, lens_l, T, 94)
    with _form(None):
        y1, q1 = _launch(ops, params, lay, xp, attp, True)
        y2, q2 = _launch(ops, params, lay, xp, attp, True)
    R = int(lay.cu[-1])
    assert torch.equal(y1, y2) and torch.equal(q1[:R], q2[:R])
