"""Per-phoneme control maps at kernel level, through the C ABI of include/fs2hip_prosody.h
(fs2amd.ops -> libfs2hip.so). Everything here is exact: a map is one f32 multiply per phoneme
(durations: rint(exp(log_d) - 1) * d, no add to contract with; pitch / energy: pred * c), so the
kernels must equal the torch formula bit for bit, a constant map must equal the scalar call, and a
broadcastable map must equal its expanded form."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPECIAL = [0.0, -1.5, 0.5, 1.0, 1.5, 2.75]  # every duration map holds these: zero, negative (clamped), fractional


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops as o
    return o


def _log_d(B, L, g):
    """log1p(k + f), integer k in [0, 10], |f| <= 0.25: an ulp of expf cannot tip the rint."""
    k = torch.randint(0, 11, (B, L), generator=g).float()
    f = (torch.rand(B, L, generator=g) - 0.5) * 0.5
    f = torch.where(k == 0, f.abs(), f)  # log1p needs k + f > -1; keep k = 0 rows at f >= 0
    return torch.log1p(k + f), k


def _d_map(B, L, g):
    m = 0.25 + 2.5 * torch.rand(B, L, generator=g)
    flat = m.view(-1)
    n = min(len(SPECIAL), flat.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = torch.tensor(SPECIAL[:n])
    return m


def _frames_ref(log_d, d_map):
    """The torch formula (modules.py:132-135) and the LengthRegulator's truncation of it."""
    dr = torch.clamp(torch.round(torch.exp(log_d) - 1) * d_map, min=0)
    frames = dr.to(torch.int64)  # int(expand_size): truncation toward zero
    return dr, torch.cumsum(frames, 1).to(torch.int32), frames.sum(1)


def _index_ref(cum, mel_len, T):
    """src(b, t) = first i with cum[b, i] > t for t < min(mel_len, T), else -1."""
    t = torch.arange(T)[None, :]
    idx = torch.searchsorted(cum.to(torch.int64).contiguous(), t.expand(cum.shape[0], T).contiguous(), right=True)
    return torch.where(t < mel_len[:, None], idx, torch.full_like(idx, -1)).to(torch.int32)


@pytest.mark.parametrize("L", [1, 7, 300, 1030, 2050])
def test_duration_map_every_entry(ops, L):
    """fs2_lr_durations_map, fs2_length_regulate_map (+ index map) and fs2_lr_fused_proj_map with and
    without the projection: d_rounded, cum and mel_len equal the torch formula exactly and all
    entries expand the same frames. L = 300: more than one element per scan thread (256 threads);
    L = 1030 > 1024: fs2_length_regulate_map leaves its padded-only kernel for the fused one;
    L = 2050 > 2048: the expand searches cum in global memory (and the fused entry refuses)."""
    B = 3
    g = torch.Generator().manual_seed(100 + L)
    log_d, k = _log_d(B, L, g)
    # torch's own exp on the CPU must round to the same integers the construction intends
    assert torch.equal(torch.round(torch.exp(log_d) - 1), k)
    d_map = _d_map(B, L, g)
    dr_ref, cum_ref, ml_ref = _frames_ref(log_d, d_map)
    ld, dm = log_d.to(DEV), d_map.to(DEV)

    cum, mel_len, dr = ops.lr_durations(ld, logpred=True, d_control=dm)
    assert torch.equal(dr.cpu(), dr_ref) and torch.equal(cum.cpu(), cum_ref) and torch.equal(mel_len.cpu(), ml_ref)

    T = int(ml_ref.max()) + 3
    im_ref = _index_ref(cum_ref, ml_ref, T)
    D = 8
    x = torch.randn(B, L, D, generator=g)
    gather = lambda xx: torch.where((im_ref >= 0)[..., None], xx[torch.arange(B)[:, None], im_ref.clamp(min=0).long()],
                                    torch.zeros(()))
    out, ml, im, dr2 = ops.length_regulate(x.to(DEV), ld, T, return_index_map=True, d_control=dm)
    assert torch.equal(dr2.cpu(), dr_ref) and torch.equal(ml.cpu(), ml_ref) and torch.equal(im.cpu(), im_ref)
    assert torch.equal(out.cpu(), gather(x))
    # without max_len: the durations launch, the host read of max(mel_len), the expand
    out3, ml3, dr3 = ops.length_regulate(x.to(DEV), ld, None, d_control=dm)
    assert torch.equal(dr3.cpu(), dr_ref) and torch.equal(out3.cpu(), gather(x)[:, :int(ml_ref.max())])

    lens = mel_len  # the decoder's lengths: every expanded frame
    if L > 2048:
        with pytest.raises(RuntimeError, match="fs2_lr_fused_proj_map"):
            ops.lr_fused(x.to(DEV), lens, T, dur=ld, logpred=True, d_control=dm)
        return
    pout, lay, cum_f, ml_f, dr_f = ops.lr_fused(x.to(DEV), lens, T, dur=ld, logpred=True, d_control=dm)
    assert torch.equal(dr_f.cpu(), dr_ref) and torch.equal(cum_f.cpu(), cum_ref) and torch.equal(ml_f.cpu(), ml_ref)
    rows = int(ml_ref.sum())
    valid = im_ref >= 0
    packed = lambda full: full[valid]  # frames in (b, t) order = the packed rows
    assert torch.equal(pout[:rows].cpu(), packed(gather(x)))
    # with the projection (D = 256 as the decoder's; NP = 8 columns): the same frames, and the
    # projected rows bf16(proj_src[src] + proj_pe[t])
    D2, NP = 256, 8
    x2 = torch.randn(B, L, D2, generator=g).to(torch.bfloat16)
    psrc = torch.randn(B * L, NP, generator=g)
    ppe = torch.randn(T, NP, generator=g)
    r = ops.lr_fused(x2.to(DEV), lens, T, dur=ld, logpred=True, d_control=dm, proj=(psrc.to(DEV), ppe.to(DEV)))
    out2, _, cum2, ml2, dr2, proj = r
    assert torch.equal(dr2.cpu(), dr_ref) and torch.equal(cum2.cpu(), cum_ref) and torch.equal(ml2.cpu(), ml_ref)
    g2 = torch.where(valid[..., None], x2[torch.arange(B)[:, None], im_ref.clamp(min=0).long()],
                     torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(out2[:rows].cpu(), packed(g2))
    pr = psrc.view(B, L, NP)[torch.arange(B)[:, None], im_ref.clamp(min=0).long()] + ppe[None, :T]
    assert torch.equal(proj[:rows].cpu(), packed(pr.to(torch.bfloat16)))


@pytest.mark.parametrize("c", [0.8, 1.0, 1.3])
def test_constant_duration_map_equals_scalar(ops, c):
    B, L, D = 3, 300, 256
    g = torch.Generator().manual_seed(7)
    ld = _log_d(B, L, g)[0].to(DEV)
    dm = torch.full((B, L), c, device=DEV)
    a, b = ops.lr_durations(ld, logpred=True, d_control=c), ops.lr_durations(ld, logpred=True, d_control=dm)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    T = int(a[1].max()) + 1
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(B, L, D, generator=g).to(DEV, dt)
        r = ops.length_regulate(x, ld, T, return_index_map=True, d_control=c)
        s = ops.length_regulate(x, ld, T, return_index_map=True, d_control=dm)
        assert all(torch.equal(u, v) for u, v in zip(r, s))
        lens, rows = r[1], int(r[1].sum())  # the packed rows past the layout's are not written
        psrc, ppe = torch.randn(B * L, 8, generator=g).to(DEV), torch.randn(T, 8, generator=g).to(DEV)
        for proj in (None, (psrc, ppe)):
            r = ops.lr_fused(x, lens, T, dur=ld, logpred=True, d_control=c, proj=proj)
            s = ops.lr_fused(x, lens, T, dur=ld, logpred=True, d_control=dm, proj=proj)
            assert torch.equal(r[0][:rows], s[0][:rows]) and all(torch.equal(u, v) for u, v in zip(r[2:5], s[2:5]))
            if proj is not None:
                assert torch.equal(r[5][:rows], s[5][:rows])


@functools.lru_cache(maxsize=1)
def _packs():
    from fs2amd.model import FastSpeech2
    from fs2amd.synth_weights import fill_module
    from _common import configs

    pc, mc, _ = configs()
    m = FastSpeech2(pc, mc)
    fill_module(m, seed=0)
    m = m.to("cuda").eval()
    return m.set_precision("bf16", "bf16x3").packed("cuda")


def _vp_inputs(B, L, lens, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(B * 100 + L)
    x = torch.randn(B, L, 256, generator=g).to(DEV, dtype)
    cmap = (0.5 + 1.5 * torch.rand(B, L, generator=g)).to(DEV)
    tgt = torch.randn(B, L, generator=g).to(DEV)
    return x, torch.tensor(lens, device=DEV), cmap, tgt


VP_SHAPES = [(3, 37, [37, 1, 20]), (3, 5, [5, 3, 0])]


@pytest.mark.parametrize("B,L,lens", VP_SHAPES)
def test_vp_fused_control_map(ops, B, L, lens):
    """fs2_vp_fused_map against the kernel's own unscaled prediction (control = 1): pred == pred_1 *
    map and x_out == bf16(x + table[bucketize(pred_1 * map)]) exactly, for the pitch group of the
    duration + pitch launch and for the energy launch; with a target the map is unused."""
    P = _packs()
    x, lens, cmap, tgt = _vp_inputs(B, L, lens)
    for F, grp, kind in ((P.vpfused.dp, 1, "pitch"), (P.vpfused.energy, 0, "energy")):
        bins, table = P.bins[kind], P.var_table[kind]
        embedded = lambda v: (x.float() + table[torch.bucketize(v, bins)]).to(torch.bfloat16)
        p1, _ = ops.vp_fused(x, F, lens, embed=(grp, None, 1.0, bins, table))
        pm, xm = ops.vp_fused(x, F, lens, embed=(grp, None, cmap, bins, table))
        assert torch.equal(pm[grp], p1[grp] * cmap) and torch.equal(xm, embedded(p1[grp] * cmap))
        if grp == 1:
            assert torch.equal(pm[0], p1[0])  # the duration group is not scaled
        pad = torch.arange(L, device=DEV)[None, :] >= lens[:, None]
        assert bool((pm[grp][pad] == 0).all())
        pt, xt = ops.vp_fused(x, F, lens, embed=(grp, tgt, cmap, bins, table))
        assert torch.equal(pt[grp], p1[grp]) and torch.equal(xt, embedded(tgt))
        for c in (0.8, 1.0, 1.3):
            a = ops.vp_fused(x, F, lens, embed=(grp, None, c, bins, table))
            b = ops.vp_fused(x, F, lens, embed=(grp, None, torch.full((B, L), c, device=DEV), bins, table))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # broadcast forms equal their expanded [B, L] forms
        for m in (cmap[:, :1], cmap[0], cmap[0, 0]):
            a = ops.vp_fused(x, F, lens, embed=(grp, None, m, bins, table))
            b = ops.vp_fused(x, F, lens, embed=(grp, None, m.expand(B, L).contiguous(), bins, table))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L,lens", VP_SHAPES)
def test_variance_embed_and_vp_head_control_map(ops, B, L, lens, dtype):
    """fs2_variance_embed_map and fs2_vp_head_map: pred == pred_1 * map, x == x + table[bucketize(
    pred_1 * map)] exactly (f32 x; bf16 x: one rounding of the f32 sum, as the kernels do); with a
    target the map is unused; constant map == scalar; broadcast forms == expanded forms."""
    from fs2amd.runtime import variance_predictors

    P = _packs()
    x, lens, cmap, tgt = _vp_inputs(B, L, lens, dtype)
    bins, table = P.bins["pitch"], P.var_table["pitch"]
    embedded = lambda v: (x.float() + table[torch.bucketize(v, bins)]).to(dtype)
    g = torch.Generator().manual_seed(3)
    pred1 = (torch.randn(B, L, generator=g) * 4).to(DEV)

    def ve(control, target=None):
        xx, pp = x.clone(), pred1.clone()
        ops.variance_embed(xx, pp, target, control, bins, table)
        return pp, xx

    pm, xm = ve(cmap)
    assert torch.equal(pm, pred1 * cmap) and torch.equal(xm, embedded(pred1 * cmap))
    pt, xt = ve(cmap, tgt)
    assert torch.equal(pt, pred1) and torch.equal(xt, embedded(tgt))
    for c in (0.8, 1.0, 1.3):
        a, b = ve(c), ve(torch.full((B, L), c, device=DEV))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for m in (cmap[:, :1], cmap[0], cmap[0, 0]):
        a, b = ve(m), ve(m.expand(B, L).contiguous())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    # the column-split predictors' head (the fp32 model's path): duration + pitch, pitch embeds
    xb = x.to(torch.bfloat16)  # the column-split convs read bf16 rows; the head adds into x (dtype)

    def head(control, target=None):
        xx = x.clone()
        y = variance_predictors(P.vpcols.dp, xb, lens, embed=(1, xx, target, control, bins, table))
        return y, xx

    p1, _ = head(1.0)
    pm, xm = head(cmap)
    assert torch.equal(pm[0], p1[0]) and torch.equal(pm[1], p1[1] * cmap) and torch.equal(xm, embedded(p1[1] * cmap))
    pt, xt = head(cmap, tgt)
    assert torch.equal(pt[1], p1[1]) and torch.equal(xt, embedded(tgt))
    for c in (0.8, 1.0, 1.3):
        a, b = head(c), head(torch.full((B, L), c, device=DEV))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for m in (cmap[:, :1], cmap[0], cmap[0, 0]):
        a, b = head(m), head(m.expand(B, L).contiguous())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_duration_map_broadcast_forms(ops):
    B, L = 3, 7
    g = torch.Generator().manual_seed(9)
    ld = _log_d(B, L, g)[0].to(DEV)
    dm = _d_map(B, L, g).to(DEV)
    x = torch.randn(B, L, 8, generator=g).to(DEV)
    for m in (dm[:, :1], dm[0], dm[0, 0], dm[:1], dm[0, :1]):
        full = m.expand(B, L).contiguous()
        a, b = ops.lr_durations(ld, logpred=True, d_control=m), ops.lr_durations(ld, logpred=True, d_control=full)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        T = int(a[1].max())
        lens, rows = a[1], int(a[1].sum())
        a = ops.length_regulate(x, ld, T, d_control=m)
        b = ops.length_regulate(x, ld, T, d_control=full)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        a = ops.lr_fused(x, lens, T, dur=ld, logpred=True, d_control=m)
        b = ops.lr_fused(x, lens, T, dur=ld, logpred=True, d_control=full)
        assert torch.equal(a[0][:rows], b[0][:rows]) and all(torch.equal(u, v) for u, v in zip(a[2:], b[2:]))


def test_duration_map_needs_log_predictions(ops):
    """A map scales predictions: with int64 or float durations every entry refuses it (FS2_EINVAL
    through L.check), as the fused entry does without durations; bad maps raise before any launch."""
    import ctypes

    from fs2amd import _lib as L

    B, Lx, D, T = 2, 5, 8, 12
    lib = L.load()
    x = torch.zeros(B, Lx, D, device=DEV)
    dm = torch.ones(B, Lx, device=DEV)
    cum = torch.empty(B, Lx, device=DEV, dtype=torch.int32)
    ml = torch.empty(B, device=DEV, dtype=torch.int64)
    dr = torch.empty(B, Lx, device=DEV)
    out = torch.empty(B, T, D, device=DEV)
    cu = torch.empty(B + 1, device=DEV, dtype=torch.int32)
    lens = torch.full((B,), 3, device=DEV, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for kind, dur in ((L.DUR_I64, torch.ones(B, Lx, device=DEV, dtype=torch.int64)),
                      (L.DUR_F32, torch.ones(B, Lx, device=DEV))):
        calls = {
            "fs2_lr_durations_map": lambda: lib.fs2_lr_durations_map(p(dur), kind, 1.0, p(dm), B, Lx, p(cum), p(ml),
                                                                     p(dr), None),
            "fs2_length_regulate_map": lambda: lib.fs2_length_regulate_map(
                p(x), L.FS2_F32, p(dur), kind, 1.0, p(dm), B, Lx, D, T, None, p(out), L.FS2_F32, p(cum), p(ml), p(dr),
                None, None),
            "fs2_lr_fused_proj_map": lambda: lib.fs2_lr_fused_proj_map(
                p(x), L.FS2_F32, p(dur), kind, 1.0, p(dm), None, None, B, Lx, D, T, None, p(lens), p(cu), None, None,
                p(out), L.FS2_F32, p(cum), p(ml), p(dr), None, None, 0, None, None),
        }
        for name, call in calls.items():
            rc = call()
            assert rc == L.FS2_EINVAL, (name, kind, rc)
            with pytest.raises(RuntimeError, match="fs2 status 1"):
                L.check(rc, name)
        with pytest.raises(RuntimeError, match="fs2_lr_durations_map failed: fs2 status 1"):
            ops.lr_durations(dur, d_control=dm)
        with pytest.raises(RuntimeError, match="fs2_lr_fused_proj_map failed: fs2 status 1"):
            ops.lr_fused(x, lens, T, dur=dur, d_control=dm)
    # the fused entry without durations (cum / mel_len given) has nothing for a map to scale
    rc = lib.fs2_lr_fused_proj_map(p(x), L.FS2_F32, None, 0, 1.0, p(dm), p(cum), p(ml), B, Lx, D, T, None, p(lens),
                                   p(cu), None, None, p(out), L.FS2_F32, None, None, None, None, None, 0, None, None)
    assert rc == L.FS2_EINVAL
    torch.cuda.synchronize()
    ld = torch.zeros(B, Lx, device=DEV)
    with pytest.raises((ValueError, RuntimeError), match="broadcast"):
        ops.lr_durations(ld, logpred=True, d_control=torch.ones(B, Lx + 1, device=DEV))
    with pytest.raises((ValueError, RuntimeError), match="float"):
        ops.lr_durations(ld, logpred=True, d_control=torch.ones(B, Lx, device=DEV, dtype=torch.int64))
    with pytest.raises((ValueError, RuntimeError), match="HIP"):
        ops.lr_durations(ld, logpred=True, d_control=torch.ones(B, Lx))
