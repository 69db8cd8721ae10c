"""fs2_attention_bwd on the adversarial-score cases of tests/_attn_cases.py
(tests/test_gpu_attention_bwd.py): the plain float64 statement of the gradient with the
cancellation-free magnitude of every output, the per-slice error measure, a float32 torch emulation
of the kernels' algorithm with their rounding points (and with one thing wrong: the mutations), and
a direct launcher through the ctypes handle.

Error measure. The gradient of a slice can be arbitrarily small beside the terms it is summed from
(a sequence of one key has dQ = dK = 0 exactly; on late_spike dP - D cancels), so no implementation
of the algorithm meets a bound relative to max|true gradient| of the slice. The standard forward
error of a GEMM is relative to the product of the absolute values instead:
    A_Q = (P o (|dP| + |D|)) |k| / temperature
    A_K = (P o (|dP| + |D|))^T |q| / temperature
    A_V = P^T |dO|
and the error of a slice is max|got - ref| / max A per (sequence, head, slice in {Q, K, V}): a short
sequence is not hidden behind a long one, dK not behind dV.

One key. A sequence of ONE key has P = 1, O = v and dS = dP - D = dO . v - dO . v: two roundings of
the same dot product (in the bf16 kernels, of the bf16 dO against the f32 dO) whose difference is
measured against |dP| + |D| = 2 |dO . v|, which cancels itself. Where a single query row carries
the slice (packed, or dO zero on the padded rows) no maximum over rows covers a small |dO . v|:
on t64 stairs_up (f32, head 0) dO . v = 0.058 beside sum|dO_i v_i| = 74.5, and the error there is
whatever the accumulation order leaves (a float32 BLAS emulation gave 1.2e-5 on one CPU and 1.4e-5
on another, an emulation in the MFMA's step order 3.8e-6, the kernel 2.4e-5; the sequences of two
or more keys stay below 4e-6). No multiple of one implementation's figure bounds another's. For
these sequences alone |dP| and |D| are therefore taken without cancellation,
    |dP| + |D|  ->  2 |dO| |v|^T        (one key),
against which the error is bounded by the rounding of the operands and of the accumulation, and
they are reported and bounded as a class of their own (slice_err)."""
import ctypes
import functools

import torch

import _attn_cases as A

DK = A.DK
SLICES = "QKV"
DO_KINDS = ("randn", "masked")


@functools.lru_cache(maxsize=None)
def make_dout(shape, H, kind):
    """dO f32 [B, T, H*dk] from a seeded CPU generator: randn on all rows, or (masked: what
    training produces) the same zeroed on the rows >= len."""
    T, lens = A.SHAPES[shape]
    g = torch.Generator().manual_seed(77 + 10 * T + H)
    do = torch.randn(len(lens), T, H * DK, generator=g, dtype=torch.float32)
    if kind == "masked":
        do = do * (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[..., None]
    else:
        assert kind == "randn", kind
    return do


def _cols(c, h):
    H = c.H
    return (slice(h * DK, (h + 1) * DK), slice((H + h) * DK, (H + h + 1) * DK),
            slice((2 * H + h) * DK, (2 * H + h + 1) * DK))


def bwd_ref64(c, dO, packed=False):
    """Autograd of transformer/Modules.py:14-25 per sequence and head in float64 on the tensors
    after rounding to the kernel's dtype, stated plainly: P = softmax(q k^T / temperature) over the
    len valid keys for all T query rows (padded layout) or the len rows (packed), O = P v,
    D = rowsum(dO o O), dP = dO v^T, dS = P o (dP - D), dQ = dS k / temperature,
    dK = dS^T q / temperature, dV = P^T dO; keys >= len and sequences without a key get zero.
    Returns (grad, mag), both float64 [B, T, 3*H*dk] in qkv's column order (packed: rows >= len
    zero and unused); mag = the magnitudes A_Q | A_K | A_V (module docstring; a sequence of one key
    has |dP| + |D| replaced by 2 |dO| |v|^T)."""
    x = c.qkv.double()
    grad = torch.zeros(c.B, c.T, 3 * c.H * DK, dtype=torch.float64)
    mag = torch.zeros_like(grad)
    for b, n in enumerate(c.lens):
        R = n if packed else c.T
        if n == 0 or R == 0:
            continue
        for h in range(c.H):
            qs, ks, vs = _cols(c, h)
            q, k, v = x[b, :R, qs], x[b, :n, ks], x[b, :n, vs]
            do = dO[b, :R, qs].double()
            P = torch.softmax(q @ k.T / c.temperature, dim=1)
            D = (do * (P @ v)).sum(1, keepdim=True)
            dP = do @ v.T
            dS = P * (dP - D)
            grad[b, :R, qs] = dS @ k / c.temperature
            grad[b, :n, ks] = dS.T @ q / c.temperature
            grad[b, :n, vs] = P.T @ do
            if n == 1:  # one key: |dP| = |D| = |dO . v| cancels itself (module docstring)
                W = 2 * (do.abs() @ v.abs().T)
            else:
                W = P * (dP.abs() + D.abs())
            mag[b, :R, qs] = W @ k.abs() / c.temperature
            mag[b, :n, ks] = W.T @ q.abs() / c.temperature
            mag[b, :n, vs] = P.T @ do.abs()
    return grad, mag


@functools.lru_cache(maxsize=None)
def ref_for(family, shape, H, dtype, kind, packed):
    """(case, dO, grad, mag): computed once per case and shared by the tests; leave it unchanged."""
    c = A.make_case(family, shape, H, dtype)
    dO = make_dout(shape, H, kind)
    grad, mag = bwd_ref64(c, dO, packed)
    return c, dO, grad, mag


CLASSES = ("keys", "one_key")  # sequences of two or more keys / of one key (slice_err)


def slice_err(got, ref, mag, c, packed):
    """Worst max|got - ref| / max A over (sequence, head, slice), with its place (b, len, h,
    slice), separately for the sequences of two or more keys and for those of ONE key:
    {"keys": (err, at), "one_key": (err, at)}; the latter's magnitude is another (module docstring,
    bwd_ref64), so the two are not comparable. got: per-sequence list of [rows, 3*H*dk] (launch_bwd, emulate); ref: the
    same or a [B, T, ..] tensor. All T rows padded, the sequence's own rows packed. Everything must
    be finite; a slice whose magnitude is zero (a sequence without keys) must equal ref exactly."""
    worst = {k: (0.0, None) for k in CLASSES}
    for b, n in enumerate(c.lens):
        R = n if packed else c.T
        if R == 0:
            continue
        g, r, a = got[b][:R].double(), ref[b][:R].double(), mag[b][:R]
        assert bool(torch.isfinite(g).all()), ("non-finite gradient", b, n)
        cls = "one_key" if n == 1 else "keys"
        for h in range(c.H):
            for name, cs in zip(SLICES, _cols(c, h)):
                d, amax = float((g[:, cs] - r[:, cs]).abs().max()), float(a[:, cs].max())
                if amax == 0.0:
                    assert d == 0.0, ("zero-magnitude slice differs", b, n, h, name, d)
                    continue
                if d / amax > worst[cls][0]:
                    worst[cls] = (d / amax, (b, n, h, name))
    return worst


def ref_lse(c):
    """The float64 case.lse rounded to f32 [B, T, H] (+inf for a sequence without keys)."""
    return c.lse.float()


MUTATIONS = ("mask_last_key", "skip_tile0", "d_zero", "dk_no_temp", "drop_pad_rows")


def _mm(a, b, step):
    """a [M, K] @ b [K, N] as the MFMA accumulates it: `step` products at a time summed exactly
    (float64) and added to the f32 accumulator with ONE rounding. Unlike a float32 BLAS call the
    result does not depend on the CPU the test runs on, so the pinned figures hold everywhere."""
    (M, K), N = a.shape, b.shape[1]
    ns = (K + step - 1) // step
    ad, bd = torch.zeros(M, ns * step, dtype=torch.float64), torch.zeros(ns * step, N, dtype=torch.float64)
    ad[:, :K], bd[:K] = a, b
    part = torch.bmm(ad.view(M, ns, step).transpose(0, 1), bd.view(ns, step, N))  # [ns, M, N] float64
    acc = torch.zeros(M, N, dtype=torch.float32)
    for i in range(ns):
        acc = (acc.double() + part[i]).float()
    return acc


def _rowdot(do, o, ke):
    """D = rowsum(dO o O) as the dQ kernel sums it: lane group g of 4 takes the ke elements at
    g*ke of every 4*ke-column chunk, one f32 fma per element in column order, then the four
    partial sums are added pairwise ((0 + 1) + (2 + 3)). [R, dk] x [R, dk] -> [R, 1] f32."""
    R = do.shape[0]
    prod = (do.double() * o.double()).view(R, DK // (4 * ke), 4, ke).permute(0, 2, 1, 3).reshape(R, 4, DK // 4)
    part = torch.zeros(R, 4, dtype=torch.float32)
    for i in range(DK // 4):
        part = (part.double() + prod[:, :, i]).float()  # the product is exact in float64: an fma
    return ((part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3]))[:, None]


def emulate(c, dO, packed=False, mutate=None):
    """The kernels' algorithm on the CPU with their rounding points: operands in the kernel's
    dtype; every GEMM accumulated in f32 once per MFMA step (_mm: 32 products bf16, 4 f32);
    p = exp2(s * log2(e)/temperature - lse) in f32 with lse the float64 reference's rounded to f32
    (exp2 itself correctly rounded); D = rowsum(dO o O) from the ROUNDED O and the f32 dO in the
    dQ kernel's order (_rowdot); P, dS and dO rounded to the kernel's dtype before the second
    GEMMs (no rounding at all for f32). Every operation is an IEEE one of a stated order, so the
    result is the same on every CPU. mutate: one of MUTATIONS, the same with one thing wrong.
    Returns the per-sequence list of f32 [rows, 3*H*dk]."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rnd = lambda t: t.to(c.dtype).float()
    step, ke = (32, 8) if c.dtype == torch.bfloat16 else (4, 4)
    x = c.qkv.float()
    o_all = c.ref.to(c.dtype).float()
    lse_all = ref_lse(c)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    scale_log2, inv_temp = f32(1.4426950408889634) / f32(c.temperature), f32(1.0) / f32(c.temperature)
    res = []
    for b, n in enumerate(c.lens):
        R = n if packed else c.T
        g = torch.zeros(R, 3 * c.H * DK, dtype=torch.float32)
        res.append(g)
        if n == 0:
            continue
        for h in range(c.H):
            qs, ks, vs = _cols(c, h)
            q, k, v = x[b, :R, qs], x[b, :n, ks], x[b, :n, vs]
            do = dO[b, :R, qs]
            p = torch.exp2((_mm(q, k.T, step) * scale_log2 - lse_all[b, :R, h, None]).double()).float()
            if mutate == "mask_last_key":
                p[:, n - 1] = 0.0
            elif mutate == "skip_tile0":
                p[:, :A.KT] = 0.0
            D = _rowdot(do, o_all[b, :R, qs], ke)
            if mutate == "d_zero":
                D = torch.zeros_like(D)
            dor = rnd(do)
            dS = rnd(p * (_mm(dor, v.T, step) - D))
            pr = rnd(p)
            g[:, qs] = _mm(dS, k, step) * inv_temp
            if mutate == "drop_pad_rows":  # the dK / dV kernel stops at len instead of T
                dS, pr = dS * (torch.arange(R) < n)[:, None], pr * (torch.arange(R) < n)[:, None]
            g[:n, ks] = _mm(dS.T, q, step) * (1.0 if mutate == "dk_no_temp" else inv_temp)
            g[:n, vs] = _mm(pr.T, dor, step)
    return res


# ---- launching -------------------------------------------------------------------------------------
WS_TAIL = 256  # sentinel floats behind the 2*B*T*H the kernel may use


def _seqs(c, t, packed, width):
    if packed:
        cu = A.cu_of(c.lens)
        return [t[int(cu[b]):int(cu[b + 1]), :width] for b in range(c.B)]
    return [t[b * c.T:(b + 1) * c.T, :width] for b in range(c.B)]


def _rows_of(c, src, packed, width, pad, dtype, fill):
    """src [B, T, width] -> [B*T, width + pad] rows in the layout, everything else = fill."""
    t = torch.full((c.B * c.T, width + pad), fill, dtype=dtype)
    if packed:
        cu = A.cu_of(c.lens)
        for b, n in enumerate(c.lens):
            t[int(cu[b]):int(cu[b]) + n, :width] = src[b, :n].to(dtype)
    else:
        t[:, :width] = src.reshape(c.B * c.T, width).to(dtype)
    return t


def bwd_buffers(c, dev, packed, dO, lse=None, qpad=0, opad=0, dpad=0, gpad=0):
    """The device buffers of one fs2_attention_bwd call on the case (launch_bwd, the rejection
    test): qkv / out / dout rows with NaN in their extra columns (and, packed, in the rows past
    cu[B]), out = the float64 forward reference rounded to the kernel's dtype, dqkv and the ws tail
    pre-filled with the sentinel. lse: None (the kernel's own pass 1), "ref" (the float64 case.lse
    rounded to f32) or the [B*T, H] f32 buffer fs2_attention_ex wrote for the same case and
    layout."""
    B, T, H = c.B, c.T, c.H
    C, Dm = 3 * H * DK, H * DK
    nan = float("nan")
    bufs = dict(qkv=_rows_of(c, c.qkv, packed, C, qpad, c.dtype, nan).to(dev),
                out=_rows_of(c, c.ref, packed, Dm, opad, c.dtype, nan).to(dev),
                dout=_rows_of(c, dO, packed, Dm, dpad, torch.float32, nan).to(dev),
                dqkv=A.sentinel((B * T, C + gpad), torch.float32, dev),
                ws=A.sentinel((2 * B * T * H + WS_TAIL,), torch.float32, dev),
                lens=None if packed else torch.tensor(c.lens, dtype=torch.int64, device=dev),
                cu=A.cu_of(c.lens).to(dev) if packed else None, lse=None)
    if isinstance(lse, str):
        assert lse == "ref", lse
        bufs["lse"] = _rows_of(c, ref_lse(c), packed, H, 0, torch.float32, nan).to(dev)
    elif lse is not None:
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (B * T, H), (lse.dtype, lse.shape)
        bufs["lse"] = lse.to(dev)
    return bufs


def call_bwd(c, bufs, **over):
    """fs2_attention_bwd's return code on the buffers; over: arguments replaced by name (the
    rejection test). No check, no synchronisation."""
    from fs2amd import _lib as L

    lib = L.load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    a = dict(qkv=p(bufs["qkv"]), dtype=L.FS2_BF16 if c.dtype == torch.bfloat16 else L.FS2_F32,
             qkv_row_stride=bufs["qkv"].shape[1], out=p(bufs["out"]), out_row_stride=bufs["out"].shape[1],
             dout=p(bufs["dout"]), dout_row_stride=bufs["dout"].shape[1], key_lens=p(bufs["lens"]), B=c.B, T=c.T,
             H=c.H, dk=DK, temperature=float(c.temperature), dqkv=p(bufs["dqkv"]),
             dqkv_row_stride=bufs["dqkv"].shape[1], seq_cu=p(bufs["cu"]), ws=p(bufs["ws"]),
             ws_bytes=2 * c.B * c.T * c.H * 4, lse=p(bufs["lse"]))
    for k, v in over.items():
        assert k in a, k
        a[k] = p(v) if isinstance(v, torch.Tensor) else v
    stream = ctypes.c_void_p(torch.cuda.current_stream(bufs["qkv"].device).cuda_stream)
    return lib.fs2_attention_bwd(*a.values(), stream)


def launch_bwd(c, dev, packed, dO, lse=None, qpad=0, opad=0, dpad=0, gpad=0):
    """fs2_attention_bwd on the case's tensors through the ctypes handle (buffers: bwd_buffers).
    Returns (dqkv, raw): dqkv as the per-sequence list of CPU f32 [T or len, 3*H*dk]; raw = the
    whole dqkv and ws buffers on the CPU and the number of rows the layout holds."""
    from fs2amd import _lib as L

    bufs = bwd_buffers(c, dev, packed, dO, lse, qpad, opad, dpad, gpad)
    L.check(call_bwd(c, bufs), "fs2_attention_bwd")
    torch.cuda.synchronize()  # a HIP error of the launch surfaces here
    g = bufs["dqkv"].cpu()
    rows = sum(c.lens) if packed else c.B * c.T
    return _seqs(c, g, packed, 3 * c.H * DK), dict(dqkv=g, ws=bufs["ws"].cpu(), rows=rows)
