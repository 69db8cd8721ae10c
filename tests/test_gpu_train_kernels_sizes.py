"""Training-step kernels (csrc/train.hip) against float64 at the sizes training runs them at, and on
inputs whose statistics are hard for f32.

tests/test_gpu_train_kernels.py keeps every case so small that each wave or block sees at most one
row. Here every grid-stride / row loop takes several steps and every split-partial reduction sees
its full number of partials:

* res_ln / relu_ln / relu_ln_head at R = 9223 rows (forward: more than the 8192 rows of one pass;
  backward: 10 passes of 256 blocks x 4 waves, R mod 4 = 3, 256 partials in the finish kernels),
  padding that covers whole 4-row blocks, relu ties, immediate / accumulating / deferred finishes;
* bn_train at row counts with empty blocks, ragged last blocks, rows-per-block below and above the
  rows per iteration, and C = 4 / 80 / 512 / 1024 (256 / 12 / 2 / 1 row slots);
* fs2_loss at 272 000 mel quads (both grids stride), fs2_adam_flat at n > 2^20 with runs of 1-3
  element parameters, fs2_colsum below the chunk count and on a strided view.

The dropout keep mask is tests/_train_ref.py's host statement of the hash, not a readback from the
kernel; the readback must equal it bit for bit.

Tolerances are the project's own (2e-5 of the output scale for f32 outputs, 1e-2 for bf16-stored
ones, rtol 1e-4 for gamma / beta sums, 1e-3 for bias sums). The hostile-statistics tests bound each
error by max(that tolerance, 4 x floor), floor = the error of torch's CPU f32 evaluation of the
same op on the same input against float64 (_train_ref.f32_error_floor); each prints floor and
measured error (recorded in profiles/train_kernels_sizes/errors.txt).
"""
import pytest
import torch
import torch.nn.functional as F

import _train_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 256
SEED_HI = (0x1234ABCD << 32) | 0x9E3779B1  # non-zero high 32 bits


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops as o
    return o


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


class _Checks:
    """Collects every figure of a case before asserting, so a failing case still prints them all."""

    def __init__(self, tag, floors=None):
        self.tag, self.floors, self.bad = tag, floors, []

    def _tol(self, key, tol):
        fl = 0.0 if self.floors is None else self.floors[key]
        return max(tol, 4.0 * fl), fl

    def _note(self, key, fl, err, bound, ok):
        if self.floors is not None:
            print(f"ERR {self.tag} {key}: floor {fl:.3e} kernel {err:.3e} bound {bound:.3e}{'' if ok else '  FAIL'}")
        if not ok:
            self.bad.append(f"{key}: {err:.3e} > {bound:.3e}")

    def scaled(self, key, got, want, tol, ref_key=None):
        """max |got - want| <= max(tol, 4 floor) * max |want|"""
        t, fl = self._tol(ref_key or key, tol)
        sc = float(want.abs().max())
        err = float((got.detach().cpu().double() - want).abs().max()) / max(sc, 1e-300)
        self._note(key, fl, err, t, err <= t)

    def sums(self, key, got, want, rtol, atol_rel):
        """allclose(got, want, rtol, atol = atol_rel * max |want|), both widened to 4 floor if larger"""
        t, fl = self._tol(key, rtol)
        ta = max(atol_rel, 4.0 * fl)
        sc = float(want.abs().max())
        d = (got.detach().cpu().double() - want).abs()
        ok = bool((d <= t * want.abs() + ta * sc).all())
        self._note(key, fl, float(d.max()) / max(sc, 1e-300), ta, ok)

    def stats(self, key, got, want, rtol=1e-5, atol=1e-6):
        """allclose(got, want, rtol, atol), widened to 4 floor (of the scale) if larger"""
        t, fl = self._tol(key, rtol)
        sc = float(want.abs().max())
        d = (got.detach().cpu().double() - want).abs()
        ok = bool((d <= t * want.abs() + max(atol, 4.0 * fl * sc)).all())
        self._note(key, fl, float(d.max()) / max(sc, 1e-300), t, ok)

    def done(self):
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)


# ---- the three LayerNorm forms ---------------------------------------------------------------------
LN_TOL = {
    "res": {"y": 2e-5, "yb": 1e-2, "dres": 2e-5, "da": 1e-2, "dg": (1e-4, 1e-4), "dbe": (1e-4, 1e-4),
            "dbias": (1e-3, 1e-4)},
    "relu": {"y": 2e-5, "yb": 1e-2, "da": 1e-2, "dg": (1e-4, 1e-4), "dbe": (1e-4, 1e-4), "dbias": (1e-3, 1e-3)},
    "head": {"y": 2e-5, "da": 1e-2, "dg": (1e-3, 1e-3), "dbe": (1e-3, 1e-3), "dbias": (1e-3, 1e-3),
             "dhw": (1e-3, 1e-3), "dhb": (1e-3, 1e-3)},
}


def _ln_ref(form, dt, a, res, gam, bet, keep, p, rowmask, hw, hb, dy):
    """The op and its autograd gradients in dtype dt on the CPU; rows [R, 256], rowmask bool [R]."""
    A, G, Bt = (t.to(dt).requires_grad_() for t in (a, gam, bet))
    kf = keep.to(dt) / (1 - p)
    leaves = {"da": A, "dg": G, "dbe": Bt}
    if form == "res":
        Rs = res.to(dt).requires_grad_()
        leaves["dres"] = Rs
        y = F.layer_norm(A * kf + Rs, (D,), G, Bt, 1e-5)
        if rowmask is not None:
            y = y.masked_fill(rowmask[:, None], 0)
    else:
        y = F.layer_norm(torch.relu(A), (D,), G, Bt, 1e-5) * kf
        if form == "head":
            W, Hb = hw.to(dt).requires_grad_(), hb.to(dt).requires_grad_()
            leaves["dhw"], leaves["dhb"] = W, Hb
            y = y @ W + Hb
            if rowmask is not None:
                y = y.masked_fill(rowmask, 0)
    y.backward(dy.to(dt))
    out = {k: v.grad.detach() for k, v in leaves.items()}
    out["y"] = y.detach()
    out["dbias"] = out["da"].sum(0)
    return out


def _ln_case(ops, form, tag, a, gam, bet, dy, *, res=None, res_bf16=False, B=1, lens=None, rowmask=None, p=0.0,
             seed=5, salt=0, hw=None, hb=None, defer=False, hostile=False):
    """Run one LayerNorm form forward and backward on rows a [R, 256] and compare with float64."""
    R = a.shape[0]
    T = R // B
    keep = TR.keep_mask(seed, salt, R, D, p)
    if lens is not None:
        rowmask = (torch.arange(T)[None, :] >= lens[:, None]).reshape(R)
    if res_bf16:
        res = res.to(torch.bfloat16).float()
    ref = _ln_ref(form, torch.float64, a, res, gam, bet, keep, p, rowmask, hw, hb, dy)
    floors = None
    if hostile:
        r32 = _ln_ref(form, torch.float32, a, res, gam, bet, keep, p, rowmask, hw, hb, dy)
        floors = {k: TR.f32_error_floor(r32[k], ref[k]) for k in ref}
        floors["yb"] = floors["y"]
    ck = _Checks(tag, floors)
    tol = LN_TOL[form]
    dev = lambda t: None if t is None else t.to(DEV)
    sd = _seed(seed)
    names = ["dg", "dbe", "dbias"] + (["dhw", "dhb"] if form == "head" else [])
    base = {k: (torch.randn(1 if k == "dhb" else D, device=DEV) if defer else None) for k in names}
    prev = {k: (None if v is None else v.clone()) for k, v in base.items()}
    q = [] if defer else None
    got = {}
    if form == "res":
        a3, r3 = dev(a).view(B, T, D), dev(res.to(torch.bfloat16) if res_bf16 else res).view(B, T, D)
        y, yb, xh, rs = ops.res_ln_fwd(a3, r3, dev(gam), dev(bet), 1e-5, dev(lens), p, sd, salt)
        got["y"], got["yb"] = y.view(R, D), yb.view(R, D)
        out = ops.res_ln_bwd(dev(dy).view(B, T, D), xh, rs, dev(gam), dev(lens), p, sd, salt, dgamma=base["dg"],
                             dbeta=base["dbe"], dbias=base["dbias"], accumulate=defer, defer=q)
        got["dres"], got["da"] = out[0].view(R, D), out[1].view(R, D)
        got["dg"], got["dbe"], got["dbias"] = out[2:]
    elif form == "relu":
        y, yb, xh, rs = ops.relu_ln_fwd(dev(a), dev(gam), dev(bet), 1e-5, p, sd, salt)
        got["y"], got["yb"] = y, yb
        out = ops.relu_ln_bwd(dev(dy), dev(a), xh, rs, dev(gam), p, sd, salt, dgamma=base["dg"], dbeta=base["dbe"],
                              dbias=base["dbias"], accumulate=defer, defer=q)
        got["da"], got["dg"], got["dbe"], got["dbias"] = out
    else:
        m3 = None if rowmask is None else dev(rowmask).view(B, T)
        y, xh, rs = ops.relu_ln_head_fwd(dev(a).view(B, T, D), dev(gam), dev(bet), 1e-5, dev(hw), dev(hb), m3, p, sd, salt)
        assert y.shape == (B, T)
        got["y"] = y.view(R)
        out = ops.relu_ln_head_bwd(dev(dy).view(B, T), m3, dev(hw), dev(bet), dev(a).view(B, T, D), xh, rs, dev(gam), p,
                                   sd, salt, dgamma=base["dg"], dbeta=base["dbe"], dbias=base["dbias"], dhw=base["dhw"],
                                   dhb=base["dhb"], accumulate=defer, defer=q)
        got["da"] = out[0].view(R, D)
        got["dg"], got["dbe"], got["dbias"], got["dhw"], got["dhb"] = out[1:]
    if defer:
        ops.reduce_flush(q, xh)
    torch.cuda.synchronize()
    for k, t in tol.items():
        if isinstance(t, tuple):
            want = ref[k] if prev[k] is None else ref[k] + prev[k].cpu().double()
            ck.sums(k, got[k], want, *t)
        else:
            ck.scaled(k, got[k], ref["y"] if k == "yb" else ref[k], t)
    assert all(bool(torch.isfinite(v.float()).all()) for v in got.values()), tag
    if rowmask is not None and form == "res":  # padding rows: exactly zero, forward and backward
        m = rowmask.to(DEV)
        for k in ("y", "yb", "dres", "da"):
            assert not bool(got[k][m].any()), (tag, k)
    if rowmask is not None and form == "head":
        assert not bool(got["y"][rowmask.to(DEV)].any()), tag
    ck.done()
    return got, ref, (xh, rs)


def _readback_keep(ops, form, R, p, seed, salt):
    """The kernel's own keep bits: res form a = 1, res = 0 (xhat > 0 exactly on kept elements);
    relu forms gamma = 0, beta = 1 (y != 0 exactly on kept elements)."""
    ones = torch.ones(1, R, D, device=DEV)
    g1, g0 = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    if form == "res":
        _, _, xh, _ = ops.res_ln_fwd(ones, torch.zeros_like(ones), g1, g0, 1e-5, None, p, _seed(seed), salt, want_bf16=False)
        return (xh > 0).view(R, D).cpu()
    y, _, _, _ = ops.relu_ln_fwd(ones.view(R, D), g0, g1, 1e-5, p, _seed(seed), salt, want_bf16=False)
    return (y != 0).cpu()


R_BIG, B_BIG, T_BIG = 9223, 23, 401


def _lens_big():
    g = torch.Generator().manual_seed(40)
    lens = torch.randint(1, T_BIG + 1, (B_BIG,), generator=g)
    lens[0], lens[1], lens[2] = T_BIG, 1, 0
    lens[3] = 100  # 301 padding rows: whole 4-row blocks take the masked path in some passes only
    return lens


@pytest.mark.parametrize("p,res_bf16,seed", [(0.0, False, 1234567), (0.1, False, SEED_HI), (0.0, True, 7),
                                             (0.1, True, 1234567)])
def test_res_ln_many_passes(ops, p, res_bf16, seed):
    torch.manual_seed(41)
    a, res, dy = torch.randn(R_BIG, D), torch.randn(R_BIG, D), torch.randn(R_BIG, D)
    gam, bet = 1 + 0.1 * torch.randn(D), 0.1 * torch.randn(D)
    lens, salt = _lens_big(), 7
    if p > 0:
        assert torch.equal(_readback_keep(ops, "res", R_BIG, p, seed, salt), TR.keep_mask(seed, salt, R_BIG, D, p))
    kw = dict(res=res, res_bf16=res_bf16, B=B_BIG, lens=lens, p=p, seed=seed, salt=salt)
    got, ref, (xh, rs) = _ln_case(ops, "res", f"res_ln p={p}", a, gam, bet, dy, **kw)
    # accumulate=True: a second immediate call adds
    dev = lambda t: t.to(DEV)
    ops.res_ln_bwd(dev(dy).view(B_BIG, T_BIG, D), xh, rs, dev(gam), dev(lens), p, _seed(seed), salt, dgamma=got["dg"],
                   dbeta=got["dbe"], dbias=got["dbias"], accumulate=True)
    torch.cuda.synchronize()
    ck = _Checks(f"res_ln accumulate p={p}")
    for k, (rt, at) in (("dg", (1e-4, 1e-4)), ("dbe", (1e-4, 1e-4)), ("dbias", (1e-3, 1e-4))):
        ck.sums(k, got[k], 2 * ref[k], rt, at)
    ck.done()
    # defer= (partials only, reduce_flush afterwards), accumulating into existing gradients
    _ln_case(ops, "res", f"res_ln defer p={p}", a, gam, bet, dy, defer=True, **kw)


def _relu_input(seed):
    torch.manual_seed(seed)
    a = torch.randn(R_BIG, D)
    a[torch.rand(R_BIG, D) < 0.01] = 0.0  # the relu tie: a == 0 passes no gradient
    gam, bet = 1 + 0.1 * torch.randn(D), 0.1 * torch.randn(D)
    return a, gam, bet


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("defer", [False, True])
def test_relu_ln_many_passes(ops, p, defer):
    a, gam, bet = _relu_input(42)
    dy = torch.randn(R_BIG, D)
    seed, salt = SEED_HI, 11
    if p > 0:
        assert torch.equal(_readback_keep(ops, "relu", R_BIG, p, seed, salt), TR.keep_mask(seed, salt, R_BIG, D, p))
    got, _, _ = _ln_case(ops, "relu", f"relu_ln p={p} defer={defer}", a, gam, bet, dy, p=p, seed=seed, salt=salt, defer=defer)
    assert not bool(got["da"][(a == 0).to(DEV)].any())


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("defer", [False, True])
def test_relu_ln_head_many_passes(ops, p, defer):
    a, gam, bet = _relu_input(43)
    hw, hb = torch.randn(D) / 16, 0.3 * torch.randn(1)
    mask = torch.rand(B_BIG, T_BIG) < 0.2
    mask[5] = True  # one fully masked sequence
    dout = torch.randn(R_BIG)
    got, _, _ = _ln_case(ops, "head", f"relu_ln_head p={p} defer={defer}", a, gam, bet, dout, B=B_BIG,
                         rowmask=mask.reshape(R_BIG), p=p, seed=77, salt=5, hw=hw, hb=hb, defer=defer)
    assert not bool(got["da"][(a == 0).to(DEV)].any())


# ---- hostile statistics: LayerNorm ------------------------------------------------------------------
R_LN = 1031


def _hostile_rows(kind):
    g = torch.Generator().manual_seed(50)
    x = torch.randn(R_LN, D, generator=g)
    if kind == "mean1e3":
        return x + 1e3
    if kind == "outlier":
        x[torch.arange(R_LN), torch.randint(0, D, (R_LN,), generator=g)] = 3e4
        return x
    if kind == "constant":  # exactly constant rows (variance 0), both signs and zero; the rest plain
        c = torch.randn(R_LN, generator=g) * 3
        c[::7] = 0.0
        const = torch.arange(R_LN) % 2 == 0
        x[const] = c[const, None].expand(-1, D)
        return x
    return x * {"tiny": 1e-6, "huge": 1e6}[kind]


@pytest.mark.parametrize("kind", ["mean1e3", "outlier", "constant", "tiny", "huge"])
@pytest.mark.parametrize("form", ["res", "relu", "head"])
def test_ln_hostile_statistics(ops, form, kind):
    a = _hostile_rows(kind)
    torch.manual_seed(51)
    gam, bet = 1 + 0.1 * torch.randn(D), 0.1 * torch.randn(D)
    kw = {}
    if form == "res":
        kw["res"] = torch.zeros(R_LN, D)
    if form == "head":
        kw.update(hw=torch.randn(D) / 16, hb=0.3 * torch.randn(1))
    dy = torch.randn(R_LN) if form == "head" else torch.randn(R_LN, D)
    got, ref, (xh, rs) = _ln_case(ops, form, f"ln_{form} {kind}", a, gam, bet, dy, hostile=True, **kw)
    if kind == "constant":  # variance 0: xhat = 0 and rstd = eps^-1/2 on the constant rows
        const = (torch.arange(R_LN) % 2 == 0).to(DEV)
        assert not bool(xh.view(R_LN, D)[const].any())
        assert float((rs[const] * 1e-5 ** 0.5 - 1).abs().max()) <= 2e-5


# ---- BatchNorm on batch statistics ------------------------------------------------------------------
def _bn_ref(dt, z, g, b, res, use_tanh, keep, p, dy):
    Z, G, Bt = (t.to(dt).requires_grad_() for t in (z, g, b))
    C = z.shape[1]
    rm, rv = torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt)
    v = F.batch_norm(Z, rm, rv, G, Bt, True, 0.1, 1e-5)
    if use_tanh:
        v = torch.tanh(v)
    y = v * keep.to(dt) / (1 - p)
    if res is not None:
        y = y + res.to(dt)
    y.backward(dy.to(dt))
    with torch.no_grad():
        _, mean, rstd = torch.native_batch_norm(z.to(dt), None, None, None, None, True, 0.1, 1e-5)
    return {"y": y.detach(), "rm": rm, "rv": rv, "mean": mean, "rstd": rstd, "dz": Z.grad, "dg": G.grad, "dbe": Bt.grad}


def _bn_case(ops, tag, z, use_tanh, p, with_res, seed=77, salt=3, hostile=False):
    R, C = z.shape
    g0 = torch.Generator().manual_seed(60 + C)
    g, b = 1 + 0.1 * torch.randn(C, generator=g0), 0.1 * torch.randn(C, generator=g0)
    res = torch.randn(R, C, generator=g0) if with_res else None
    dy = torch.randn(R, C, generator=g0)
    keep = TR.keep_mask(seed, salt, R, C, p)
    ref = _bn_ref(torch.float64, z, g, b, res, use_tanh, keep, p, dy)
    floors = None
    if hostile:
        r32 = _bn_ref(torch.float32, z, g, b, res, use_tanh, keep, p, dy)
        floors = {k: TR.f32_error_floor(r32[k], ref[k]) for k in ref}
        floors["yb"] = floors["y"]
    ck = _Checks(tag, floors)
    dev = lambda t: None if t is None else t.to(DEV)
    sd = _seed(seed)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    yb, yf, mean, rstd = ops.bn_train_fwd(dev(z), dev(g), dev(b), 1e-5, 0.1, rm, rv, use_tanh, p, sd, salt,
                                          residual=dev(res), want_bf16=True, want_f32=True)
    if p > 0:  # the kernel's own keep bits (gamma = 0, beta = 1: y != 0 exactly on kept elements)
        _, kf, _, _ = ops.bn_train_fwd(dev(z), torch.zeros(C, device=DEV), torch.ones(C, device=DEV), 1e-5, 0.1, None, None,
                                       True, p, sd, salt, want_bf16=False, want_f32=True)
        assert torch.equal((kf != 0).cpu(), keep), tag
    dz, dg, dbe = ops.bn_train_bwd(dev(dy), dev(z), dev(g), dev(b), mean, rstd, use_tanh, p, sd, salt)
    dg1, dbe1 = dg.clone(), dbe.clone()
    ops.bn_train_bwd(dev(dy), dev(z), dev(g), dev(b), mean, rstd, use_tanh, p, sd, salt, dgamma=dg, dbeta=dbe,
                     accumulate=True)
    torch.cuda.synchronize()
    ck.scaled("y", yf, ref["y"], 2e-5)
    ck.scaled("yb", yb, ref["y"], 1e-2)
    # the running stats at the old test's allclose(rtol 1e-5, atol 1e-6); the saved mean / rstd, which the
    # running stats are made of (rv = 0.9 + 0.1 var hides a small variance), at the same
    for k, got in (("rm", rm), ("rv", rv), ("mean", mean), ("rstd", rstd)):
        ck.stats(k, got, ref[k])
    ck.scaled("dz", dz, ref["dz"], 1e-2)
    ck.sums("dg", dg1, ref["dg"], 1e-4, 1e-4)
    ck.sums("dbe", dbe1, ref["dbe"], 1e-4, 1e-4)
    if not hostile:
        ck.sums("dg", dg, 2 * ref["dg"], 1e-4, 1e-4)
        ck.sums("dbe", dbe, 2 * ref["dbe"], 1e-4, 1e-4)
    for t in (yf, yb, mean, rstd, dz, dg, dbe):
        assert bool(torch.isfinite(t.float()).all()), tag
    ck.done()


@pytest.mark.parametrize("R,C,use_tanh,p,with_res", [
    (257, 512, True, 0.5, False),        # 256 blocks x 2 rows: blocks 129..255 are empty
    (256 * 3 + 5, 80, False, 0.5, True),  # 4 rows per block < 12 row slots, ragged last block
    (3333, 512, True, 0.0, False),       # 14 rows per block over 2 row slots: 7 loop steps
    (3333, 512, False, 0.5, True),
    (3333, 80, True, 0.5, False),        # 14 rows over 12 row slots: slots 0, 1 take two rows
    (3333, 80, False, 0.0, True),
    (1500, 1024, True, 0.5, False),      # one row slot
    (3333, 4, True, 0.5, False),         # 256 row slots, one column group; finish block mostly past 2C
    (3333, 4, False, 0.0, True),
])
def test_bn_train_many_rows(ops, R, C, use_tanh, p, with_res):
    g = torch.Generator().manual_seed(R + C)
    z = torch.randn(R, C, generator=g) * 2 + 0.5
    _bn_case(ops, f"bn R={R} C={C}", z, use_tanh, p, with_res, seed=SEED_HI if C == 80 else 77)


def _hostile_bn(kind):
    R, C = 3333, 80
    g = torch.Generator().manual_seed(61)
    if kind == "mean100":
        return 100 + 0.01 * torch.randn(R, C, generator=g)
    z = torch.randn(R, C, generator=g) * 2 + 0.5
    if kind.startswith("row0+"):
        z[0] += float(kind[5:])
    elif kind == "row0col7":
        z[0, 7] += 300.0
    elif kind == "constcol":
        z[:, 13] = 0.7
    return z


@pytest.mark.parametrize("kind", ["mean100", "row0+10", "row0+50", "row0+300", "row0col7", "constcol"])
def test_bn_hostile_statistics(ops, kind):
    """Row 0 far from the column mean: sums shifted by K_c = z[0][c] lose the variance to
    cancellation inside the f32 partial sums; per-block (mean, M2) merged in double does not."""
    _bn_case(ops, f"bn {kind}", _hostile_bn(kind), False, 0.0, False, hostile=True)


# ---- fused loss ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_level", [False, True])
def test_loss_many_quads(ops, frame_level, monkeypatch):
    """fs2_loss_fwd / _bwd at 8 x 1700 x 80 (272 000 mel quads: above the 65 536 threads of the
    forward grid and the 262 144 of the backward's) against float64 on the CPU (losses rtol 1e-5,
    gradients within 1e-6 of each gradient's scale) and the f32 torch route."""
    from fs2amd.loss import FastSpeech2Loss
    import numpy as np

    g = torch.Generator().manual_seed(70)
    B, L, T, C = 8, 150, 1700, 80
    lvl = "frame_level" if frame_level else "phoneme_level"
    pc = {"preprocessing": {"pitch": {"feature": lvl}, "energy": {"feature": "phoneme_level"}}}
    src_lens = torch.tensor([150, 10, 1, 77, 120, 33, 149, 64])
    mel_lens = torch.tensor([1700, 300, 3, 0, 1699, 1024, 777, 1333])  # utterance 3: no valid frame
    src_valid = torch.arange(L)[None] < src_lens[:, None]
    mel_valid = torch.arange(T)[None] < mel_lens[:, None]
    PL = T if frame_level else L
    rn = lambda *s: torch.randn(*s, generator=g)
    mel, post, pp, ep, ld = rn(B, T, C), rn(B, T, C), rn(B, PL), rn(B, L), rn(B, L)
    tgt, ptg, etg = rn(B, T + 9, C), rn(B, PL), rn(B, L)  # the target is longer than the prediction
    dur = torch.randint(0, 30, (B, L), generator=g)
    for b, t, c in ((0, 0, 0), (0, 1699, 79), (4, 1698, 3), (6, 500, 40)):  # exact-zero errors
        tgt[b, t, c] = mel[b, t, c]
        post[b, t, (c + 1) % C] = tgt[b, t, (c + 1) % C]
    w = (1.0, 0.0, 0.5, 0.0, 0.0, 0.25)

    def run(fused):
        monkeypatch.setenv("FS2_LOSS_FUSED", "1" if fused else "0")
        leaves = [t.to(DEV).requires_grad_() for t in (mel, post, pp, ep, ld)]
        inputs = (None,) * 9 + (tgt.to(DEV), mel_lens.to(DEV), T + 9, ptg.to(DEV), etg.to(DEV), dur.to(DEV))
        preds = (*leaves, None, (~src_valid).to(DEV), (~mel_valid).to(DEV), None, None)
        losses = FastSpeech2Loss(pc, None)(inputs, preds)
        sum(wi * li for wi, li in zip(w, losses) if wi).backward()
        torch.cuda.synchronize()
        return [float(x) for x in losses], [t.grad.detach().cpu() for t in leaves]

    lf, gf = run(True)
    lt, gt = run(False)
    # float64
    lv = [t.double().requires_grad_() for t in (mel, post, pp, ep, ld)]
    tg = tgt.double()[:, :T]
    pm = mel_valid if frame_level else src_valid
    l_mel, l_post = (lv[0] - tg).abs()[mel_valid].mean(), (lv[1] - tg).abs()[mel_valid].mean()
    l_p = ((lv[2] - ptg.double()) ** 2)[pm].mean()
    l_e = ((lv[3] - etg.double()) ** 2)[src_valid].mean()
    l_d = ((lv[4] - torch.log(dur.double() + 1)) ** 2)[src_valid].mean()
    l64 = [l_mel + l_post + l_d + l_p + l_e, l_mel, l_post, l_p, l_e, l_d]
    sum(wi * li for wi, li in zip(w, l64) if wi).backward()
    print("losses fused", lf, "float64", [float(x) for x in l64])
    np.testing.assert_allclose(lf, [float(x) for x in l64], rtol=1e-5)
    np.testing.assert_allclose(lf, lt, rtol=1e-5)
    for name, a, b32, leaf in zip(("mel", "postnet", "pitch", "energy", "log_d"), gf, gt, lv):
        want = leaf.grad
        err, sc = float((a.double() - want).abs().max()), float(want.abs().max())
        print(f"loss grad {name}: err {err:.3e} scale {sc:.3e}")
        assert sc > 0 and err <= 1e-6 * sc, (name, err, sc)
        assert float((a - b32).abs().max()) <= 1e-6 * max(1e-3, float(b32.abs().max())), name
    assert not bool(gf[0][~mel_valid].any()) and not bool(gf[1][~mel_valid].any())
    assert float(gf[0][0, 0, 0]) == 0.0 and float(gf[1][0, 0, 1]) == 0.0  # zero error: zero L1 gradient


# ---- clip + Adam -----------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [True, False])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_flat_runs_of_tiny_parameters(ops, capturable, wd):
    """fs2_adam_flat at n > 2^20 (the norm kernel's 1024 x 256 x 4 floats stride) over a layout with
    runs of 1-3 element parameters (a thread's next group lies several descriptors on), ragged ends
    and gaps, one of them wider than the 16-byte rounding; against clip_grad_norm_ +
    torch.optim.Adam(fused=True) exactly as tests/test_gpu_train_kernels.py does."""
    from fs2amd.optimizer import ScheduledOptim

    torch.manual_seed(9)
    shapes = [(1,), (3,), (2,), (5,), (4093,), (1,), (1,), (70001,), (9,), (1100, 1024), (7,)]
    ps = [torch.randn(s, device=DEV) * 0.1 for s in shapes]
    tc = {"optimizer": {"betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": wd, "warm_up_step": 4000,
                        "anneal_steps": [], "anneal_rate": 0.3, "grad_acc_step": 1, "grad_clip_thresh": 1.0}}
    mc = {"transformer": {"encoder_hidden": 256}}

    class M(torch.nn.Module):
        def __init__(self, init):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in init])

    ma, mb = M(ps), M(ps)
    oa = ScheduledOptim(ma, tc, mc, 0, capturable=capturable)
    ob = ScheduledOptim(mb, tc, mc, 0, capturable=capturable)
    offs, n = [], 0
    for i, p in enumerate(ma.parameters()):
        offs.append(n)
        n += (p.numel() + 3) // 4 * 4 + (8 if i == 8 else 0)  # after (9,): a gap of two more groups
    assert n > 1 << 20
    flat = torch.zeros(n, device=DEV)
    for p, off in zip(ma.parameters(), offs):
        p.grad = flat[off:off + p.numel()].view_as(p)
    used = torch.zeros(n, dtype=torch.bool, device=DEV)
    for p, off in zip(ma.parameters(), offs):
        used[off:off + p.numel()] = True
    for step in range(3):
        gs = [torch.randn(s, device=DEV) * (3.0 if step == 0 else 0.001) for s in shapes]
        for p, g in zip(ma.parameters(), gs):
            p.grad.copy_(g)
        for p, g in zip(mb.parameters(), gs):
            p.grad = g.clone()
        oa._update_learning_rate()
        oa.flat_step(flat, list(ma.parameters()), 1.0)
        ob._update_learning_rate()
        torch.nn.utils.clip_grad_norm_(mb.parameters(), 1.0)
        ob._optimizer.step()
        torch.cuda.synchronize()
        for i, (pa, pb) in enumerate(zip(ma.parameters(), mb.parameters())):
            assert torch.allclose(pa.grad, pb.grad, rtol=1e-5, atol=1e-7), (step, i)
            assert torch.allclose(pa, pb, rtol=1e-5, atol=1e-7), (step, i)
            sa, sb = oa._optimizer.state[pa], ob._optimizer.state[pb]
            assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-9), (step, i)
            assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-12), (step, i)
            assert float(sa["step"]) == float(sb["step"]) == step + 1
        assert not flat[~used].any()


# ---- column sums -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,N,W", [(1, 768, 768), (5, 80, 80), (1111, 768, 1024), (9223, 256, 256), (5, 256, 512)])
def test_colsum_few_rows_and_strided(ops, dtype, R, N, W):
    """fs2_colsum with fewer rows than chunks (R = 1, 5), more than 64 x 128 rows, a partial
    256-column stripe (N = 80) and a strided-row view (row stride W > N)."""
    torch.manual_seed(R + N)
    buf = torch.randn(R, W).to(dtype)
    x = buf.to(DEV)[:, :N]
    assert W == N or not x.is_contiguous()
    ref = buf[:, :N].double().sum(0)
    out = ops.colsum(x)
    torch.cuda.synchronize()
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-5, atol=1e-4)
    out2 = ops.colsum(x, out=out.clone(), accumulate=True)
    torch.cuda.synchronize()
    assert torch.allclose(out2.cpu().double(), 2 * ref, rtol=1e-5, atol=2e-4)
