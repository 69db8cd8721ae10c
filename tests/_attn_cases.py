"""Adversarial-score cases for fs2_attention_ex (tests/test_gpu_attention_forms.py and its child
tests/attn_forms_child.py): q / k / v generators whose SCALED SCORES have a stated shape, the plain
CPU statement of transformer/Modules.py:14-25 (float64 reference, float32 for the conditioning
test), and a direct launcher through the ctypes handle.

Scores are built as a rank-one term along a per-head +-1 direction u plus noise orthogonal to u:
    q_i = a_i u + nq_i,   k_j = f_j (temperature / 128) u + nk_j      (nq, nk orthogonal to u)
so that q_i . k_j / temperature = a_i f_j + N(0, (sq sk)^2): f is the family's profile IN NATS over
the keys and a selects the queries that see it. A second direction u2 (orthogonal to u; the noise
is orthogonal to it as well) carries a profile only the padded query rows t >= len see (b_i = 1
there): data that moves THEIR running max without touching a valid query's scores.

Every case is checked on the CPU before anything is launched: the float64 scores recomputed from
the tensors AFTER rounding to the kernel's dtype must have the family's property (check_family),
which proves that the case reaches the kernel path it is meant to."""
import ctypes
import functools
import math

import torch

DK = 128
KT = 64                      # keys per tile of every kernel form
LN2 = math.log(2.0)
LAZY_NATS = 8.0 * LN2        # attn32_kernel's lazy-max threshold (kLazy = 8 in the log2 domain)
TEMP = float(128 ** 0.5)

LENS_449 = [449, 0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448]
LENS_64 = [64, 63, 33, 32, 17, 16, 1, 0]
LENS_2048 = [2048, 0, 1, 256, 257, 511, 512, 513, 1793, 2047]
SHAPES = {"t449": (449, LENS_449), "t64": (64, LENS_64), "t1": (1, [1, 0]), "t2048": (2048, LENS_2048)}

FAMILIES = ["randn", "stairs_up", "creep_up", "stairs_down", "late_spike", "late_spike_tile_end", "mixed_wave",
            "stairs_up_t3"]
STEP_UP, STEP_CREEP, STEP_DOWN, SPIKE = 8.5, 4.6, 9.0, 12.0


def rise_tiles(ntiles):
    """stairs_up: up to 8 rising tiles spread evenly over the sequence's tiles (never tile 0)."""
    nr = min(8, ntiles - 1)
    return sorted({(k + 1) * ntiles // (nr + 1) for k in range(nr)} - {0})


def _profile(family, T, n):
    """f_j in nats over the keys of a sequence of n keys in a [.., T, ..] batch."""
    f = torch.zeros(T, dtype=torch.float64)
    tile = torch.arange(T) // KT
    if family in ("stairs_up", "stairs_up_t3"):
        for r in rise_tiles((T + KT - 1) // KT):
            f += STEP_UP * (tile >= r)
    elif family == "creep_up":
        f = STEP_CREEP * tile.double()
    elif family == "stairs_down":
        f = -STEP_DOWN * tile.double()
    elif family in ("late_spike", "mixed_wave") and n > 0:
        f[n - 1] = SPIKE
    elif family == "late_spike_tile_end" and n > 0:
        f[(n // KT) * KT - 1 if n >= KT else n - 1] = SPIKE
    if family in ("stairs_up", "stairs_up_t3", "creep_up") and n > 0:
        # the sequence's top step at 0 nats: the keys that carry the softmax have small |score|, so
        # the f32 rounding of a score (an ulp of |s|) stays far below the f32 output bound
        f = f - f[n - 1]
    return f


def spike_key(family, n):
    if family == "late_spike_tile_end" and n >= KT:
        return (n // KT) * KT - 1
    return n - 1


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(family, shape, H=2, dtype="bf16", pad_trip=False):
    """The case's tensors (CPU, rounded to dtype), its float64 reference and the family's property
    asserted on the recomputed scores. pad_trip: the padded query rows t >= len get the stairs_up
    profile along u2 (their running max trips the lazy threshold on tiles where a valid query's
    does not)."""
    T, lens = SHAPES[shape]
    B = len(lens)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    seed = 1000 * FAMILIES.index(family) + 10 * T + H + (5 if pad_trip else 0)
    g = torch.Generator().manual_seed(seed)
    temperature = 3.0 if family == "stairs_up_t3" else TEMP
    C = 3 * H * DK
    qkv = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    if family != "randn" or pad_trip:
        sq = sk = 1.0 if family in ("randn", "late_spike", "late_spike_tile_end", "mixed_wave") else 0.5
        for h in range(H):
            u = torch.randint(0, 2, (DK,), generator=g).double() * 2 - 1
            s2 = torch.ones(DK, dtype=torch.float64)
            s2[torch.randperm(DK, generator=g)[:DK // 2]] = -1
            u2 = u * s2  # u . u2 = sum(s2) = 0
            proj = lambda n: n - (n @ u)[..., None] * u / DK - (n @ u2)[..., None] * u2 / DK
            qs, ks = slice(h * DK, (h + 1) * DK), slice((H + h) * DK, (H + h + 1) * DK)
            nq, nk = proj(qkv[..., qs]) * sq, proj(qkv[..., ks]) * sk
            for b, n in enumerate(lens):
                t = torch.arange(T)
                a = torch.ones(T, dtype=torch.float64) if family != "randn" else torch.zeros(T, dtype=torch.float64)
                if family == "mixed_wave":
                    a = (t % 32 == 5).double()
                f = _profile(family, T, n)
                if family in ("late_spike", "late_spike_tile_end", "mixed_wave") and n > 0:
                    nk[b, spike_key(family, n)] = 0.0  # the spike is +SPIKE nats for every query exactly
                bq = (t >= n).double() if pad_trip else torch.zeros(T, dtype=torch.float64)
                gk = _profile("stairs_up", T, n) if pad_trip else torch.zeros(T, dtype=torch.float64)
                if pad_trip:
                    a = a * (t < n)
                nq[b] += a[:, None] * u + bq[:, None] * u2
                nk[b] += (f[:, None] * u + gk[:, None] * u2) * (TEMP / DK)
            qkv[..., qs], qkv[..., ks] = nq, nk
    if temperature != TEMP:
        qkv[..., :H * DK] *= temperature / TEMP  # the same nats at another temperature
    c = Case()
    c.family, c.shape, c.H, c.dtype, c.T, c.B, c.lens = family, shape, H, tdt, T, B, list(lens)
    c.temperature = temperature
    c.qkv = qkv.to(tdt)
    c.ref, c.lse, c.stats = attn_cpu(c.qkv, c.lens, H, temperature, torch.float64)
    check_family(c, pad_trip)
    return c


def attn_cpu(qkv, lens, H, temperature, dtype):
    """transformer/Modules.py:14-25 per sequence and head in `dtype` on the CPU: out [B, T, H*dk]
    (all T query rows; zeros for a sequence without keys), lse [B, T, H] = log2(sum_j exp(s_ij))
    (+inf without keys), and in float64 per (b, h) with keys the stats check_family reads, in
    nats: tm [T, ntiles] row maxima of every 64-key tile, span = max - min score, s_at = the
    scores themselves (T <= 512 only)."""
    x = qkv.to(dtype)
    B, T, _ = x.shape
    out = torch.zeros(B, T, H * DK, dtype=dtype)
    lse = torch.full((B, T, H), float("inf"), dtype=dtype)
    stats = {}
    for b, n in enumerate(lens):
        if n == 0:
            continue
        for h in range(H):
            q = x[b, :, h * DK:(h + 1) * DK]
            k = x[b, :n, (H + h) * DK:(H + h + 1) * DK]
            v = x[b, :n, (2 * H + h) * DK:(2 * H + h + 1) * DK]
            s = torch.matmul(q, k.transpose(0, 1)) / temperature
            out[b, :, h * DK:(h + 1) * DK] = torch.matmul(torch.softmax(s, dim=1), v)
            lse[b, :, h] = torch.logsumexp(s, dim=1) / LN2
            if dtype == torch.float64:
                nt = (n + KT - 1) // KT
                tm = torch.stack([s[:, t * KT:min((t + 1) * KT, n)].max(1).values for t in range(nt)], 1)
                stats[b, h] = dict(tm=tm, span=float(s.max() - s.min()), s_at=s)
    # the full score matrices are kept only where check_family reads them (small shapes)
    if T > 512:
        for st in stats.values():
            st["s_at"] = None
    return out, lse, stats


def lazy_trace(tm):
    """attn32_kernel's lazy running max replayed lane-locally on the tile maxima tm [T, ntiles]
    (nats): per query the number of rescales after the first tile and the largest exponent (nats)
    a p = exp(s - m_run) takes between rescales."""
    m = tm[:, 0].clone()
    nres = torch.zeros(tm.shape[0], dtype=torch.int64)
    pmax = torch.zeros(tm.shape[0], dtype=torch.float64)
    for t in range(1, tm.shape[1]):
        d = tm[:, t] - m
        over = d > LAZY_NATS
        nres += over
        pmax = torch.maximum(pmax, torch.where(over, torch.zeros_like(d), d))
        m = torch.where(over, tm[:, t], m)
    return nres, pmax


def check_family(c, pad_trip=False):
    """The family's property on the float64 scores of the rounded tensors (module docstring)."""
    fam = c.family
    for (b, h), st in c.stats.items():
        n, tm = c.lens[b], st["tm"]
        rows = slice(0, n) if pad_trip else slice(0, c.T)  # pad_trip: the property is the valid rows'
        tm = tm[rows]
        nt = tm.shape[1]
        nres, pmax = lazy_trace(tm)
        tag = (fam, c.shape, b, h, n)
        if fam in ("stairs_up", "stairs_up_t3"):
            rises = [r for r in rise_tiles((c.T + KT - 1) // KT) if r < nt]
            for r in rises:
                assert float((tm[:, r] - tm[:, :r].max(1).values).min()) >= 6.5, tag
            assert st["span"] <= 80.0, (tag, st["span"])
            assert int(nres.min()) >= len(rises), tag
        elif fam == "creep_up":
            for t in range(1, nt):
                d = tm[:, t] - tm[:, t - 1]
                assert 3.0 < float(d.min()) and float(d.max()) < LAZY_NATS, (tag, t, float(d.min()), float(d.max()))
            if nt >= 3:  # below the threshold per step, over it every second tile
                assert int(nres.min()) >= (nt - 1) // 2 and float(pmax.min()) > 3.0, tag
                assert float(pmax.max()) < LAZY_NATS, tag
        elif fam == "stairs_down":
            for t in range(1, nt):
                assert float((tm[:, t] - tm[:, t - 1]).max()) <= -7.0, (tag, t)
            assert int(nres.max()) == 0, tag
        elif fam in ("late_spike", "late_spike_tile_end", "mixed_wave") and c.T <= 512:
            j = spike_key(fam, n)
            s = st["s_at"][rows]
            other = torch.cat([s[:, :j], s[:, j + 1:]], 1)
            lead = s[:, j] - (other.max(1).values if n > 1 else torch.zeros(s.shape[0], dtype=s.dtype))
            sees = torch.ones(s.shape[0], dtype=torch.bool) if fam != "mixed_wave" else torch.arange(s.shape[0]) % 32 == 5
            if not bool(sees.any()):
                continue
            assert float((s[sees, j] - SPIKE).abs().max()) < 0.1, tag
            if n > 1:  # ... and the spike leads every other key by more than the lazy threshold
                assert float(lead[sees].min()) >= LAZY_NATS + 0.25, (tag, float(lead[sees].min()))
            if j >= KT:
                assert int(nres[sees].min()) >= 1, tag
            if bool((~sees).any()):  # the other 31 lanes of each wave: plain randn, no rescale of their own
                assert int(nres[~sees].max()) == 0, tag
        elif fam in ("late_spike", "late_spike_tile_end"):  # long shapes: the spike's tile trips
            j = spike_key(fam, n)
            if j >= KT:
                assert int(nres.min()) >= 1, tag
                assert float((tm[:, j // KT] - tm[:, :j // KT].max(1).values).min()) >= LAZY_NATS + 0.25, tag
        elif fam == "randn":
            assert int(nres.max()) == 0, tag  # the baseline never rescales after the first tile


def seq_rel_err(got, ref, lens, T, packed):
    """max over sequences of max|got - ref| / max|ref| of THAT sequence (all T rows padded, the
    sequence's own rows packed); a sequence without keys must be all zeros."""
    worst, at = 0.0, None
    for b, n in enumerate(lens):
        rows = n if packed else T
        if rows == 0:
            continue
        g, r = got[b][:rows].double(), ref[b][:rows]
        if n == 0:
            assert float(g.abs().max()) == 0.0, ("no keys: output not zero", b)
            continue
        assert bool(torch.isfinite(g).all()), ("non-finite output", b, n)
        e = float((g - r).abs().max() / r.abs().max())
        if e > worst:
            worst, at = e, (b, n)
    return worst, at


def lse_err(got, ref, lens, T, packed):
    """max |lse - ref| (log2 units) over the rows with keys; +inf exactly where there are none."""
    worst = 0.0
    for b, n in enumerate(lens):
        rows = n if packed else T
        if rows == 0:
            continue
        g = got[b][:rows].double()
        if n == 0:
            assert bool((g == float("inf")).all()), ("no keys: lse not +inf", b)
            continue
        assert bool(torch.isfinite(g).all()), ("non-finite lse", b, n)
        worst = max(worst, float((g - ref[b][:rows]).abs().max()))
    return worst


# ---- launching -------------------------------------------------------------------------------------
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5  # NaN bit patterns: no finite result can equal them


def sentinel(shape, dtype, device):
    if dtype == torch.bfloat16:
        return torch.full(shape, SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)
    return torch.full(shape, SENT32, dtype=torch.int32, device=device).view(torch.float32)


def is_sentinel(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16) == SENT16
    return t.view(torch.int32) == SENT32


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


def launch(c, dev, packed, waves=0, lse=False, qpad=0, opad=0, split=None, lens=None, T=None):
    """fs2_attention_ex on the case's tensors through the ctypes handle. Returns (out, lse, raw):
    out / lse as per-sequence lists of CPU tensors ([T or len, H*dk] / [.., H]); raw = the device
    out / lse / qkv buffers whole (sentinel checks). qpad / opad: extra columns of the qkv / out
    rows (qkv's hold NaN, out's the sentinel); packed rows past cu[B] hold NaN in qkv. split:
    None, or rows_max for the key-split form (fs2_attention_items + split_ws). lens / T: another
    bucket of the same batch (lengths clipped by the caller)."""
    from fs2amd import _lib as L

    lib = L.load()
    lens = c.lens if lens is None else lens
    T = c.T if T is None else T
    B, H = c.B, c.H
    C, D = 3 * H * DK, H * DK
    rows = B * T
    qkv = torch.full((rows, C + qpad), float("nan"), dtype=c.dtype)
    if packed:
        cu = cu_of(lens)
        for b, n in enumerate(lens):
            qkv[int(cu[b]):int(cu[b]) + n, :C] = c.qkv[b, :n]
    else:
        cu = None
        qkv[:, :C] = c.qkv[:, :T].reshape(rows, C)
    qd = qkv.to(dev)
    out = sentinel((rows, D + opad), c.dtype, dev)
    lse_d = sentinel((rows, H), torch.float32, dev) if lse else None
    lens_d = torch.tensor(lens, dtype=torch.int64, device=dev)
    cu_d = cu.to(dev) if packed else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(qd.device).cuda_stream)
    ws, ws_bytes, rows_max = None, 0, 0
    if split is not None:
        rows_max = int(split)
        ws_bytes = lib.fs2_attention_split_ws_bytes(B, T, H, rows_max)
        assert ws_bytes > 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        L.check(lib.fs2_attention_items(_ptr(cu_d), B, T, H, _ptr(ws), ws_bytes, rows_max, stream), "fs2_attention_items")
    code = L.FS2_BF16 if c.dtype == torch.bfloat16 else L.FS2_F32
    L.check(lib.fs2_attention_ex(_ptr(qd), code, C + qpad, None if packed else _ptr(lens_d), B, T, H, DK,
                                 float(c.temperature), _ptr(out), D + opad, _ptr(cu_d), _ptr(lse_d), waves, _ptr(ws),
                                 ws_bytes, rows_max, stream), "fs2_attention_ex")
    torch.cuda.synchronize()  # a HIP error of the launch surfaces here
    oc = out.cpu()
    lc = lse_d.cpu() if lse else None
    if packed:
        seq = lambda t, w: [t[int(cu[b]):int(cu[b + 1]), :w] for b in range(B)]
    else:
        seq = lambda t, w: [t[b * T:(b + 1) * T, :w] for b in range(B)]
    return seq(oc, D), (seq(lc, H) if lse else None), dict(out=oc, lse=lc, rows=int(cu[-1]) if packed else rows)
