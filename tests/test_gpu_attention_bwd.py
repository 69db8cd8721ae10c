"""fs2_attention_bwd (csrc/attention_bwd.hip: the dQ kernel and the dK / dV kernel, bf16 and exact
f32, statistics from the dQ kernel's own pass 1 or from the forward's lse, padded or packed rows)
against the plain float64 statement of the gradient, per (sequence, head, slice) on the
adversarial-score cases of tests/_attn_cases.py: the online rescale of pass 1 (stairs_up*, creep_up
move the running max on every tile), p = exp2(s - lse) with lse from elsewhere, the whole mass on
a tile's last key (late_spike*), lengths at every 32 / 64 / 128 / 256 edge, 0 and 1, padded query
rows that still feed dK / dV, the packed workspace indexing, other strides, and what the kernels
must leave alone.

Called through the ctypes handle (tests/_attn_bwd.py: launch_bwd); `out` is the float64 forward
reference rounded to the kernel's dtype, so only test_bwd_forward_lse runs the forward kernel.

Measure (tests/_attn_bwd.py): max|got - ref| / max A per (sequence, head, slice in {Q, K, V}) with
A the cancellation-free magnitude of the slice. A bound relative to max|true gradient| cannot be
met by any implementation (one key: dQ = dK = 0 exactly; late_spike: dP - D cancels).

Bounds. test_bwd_conditioning (CPU) runs an emulation of the algorithm in float32 arithmetic
with the kernels' rounding points (operands in the kernel's dtype, f32 accumulation once per MFMA
step, D from the rounded O, P / dS / dO rounded before the second GEMMs, lse = the float64
reference's in f32; _attn_bwd.emulate: IEEE operations in a stated order, the same on every CPU) on
every case the device tests use, in both layouts and with the kinds of dO they use. Its worst
errors, measured with the emulation committed here and pinned below (sequences of two or more
keys):
    EMUL_BF16 = 4.9e-3   (measured 4.864e-3: t64 mixed_wave, padded, randn dO, b 4 len 17 h 1, dK)
    EMUL_F32  = 1.9e-6   (measured 1.877e-6: t64 mixed_wave, padded, randn dO, b 3 len 32 h 1, dV)
The families' worst figures are 1.9e-3 .. 4.9e-3 (bf16) and 1.7e-7 .. 1.9e-6 (f32: the peaked
families are the high ones, a score of 12 nats carries an f32 rounding of 1e-6 in s and in lse).
The sequences of ONE key are measured against another magnitude (tests/_attn_bwd.py: in the
measure above their dS = dO . v - dO . v is set against |dO . v|, which cancels itself, and the
figure is whatever the accumulation order leaves: 2.4e-5 from the f32 kernels, 3.8e-6 from this
emulation, 1.2e-5 / 1.4e-5 from float32 BLAS on two CPUs) and have figures of their own:
    EMUL_BF16_ONE_KEY = 3.2e-3   (measured 3.149e-3: t449 randn, packed, b 2 len 1 h 1, dV)
    EMUL_F32_ONE_KEY  = 1.4e-6   (measured 1.305e-6: t64 late_spike, packed, b 6 len 1 h 0, dV)
The kernel bounds are BOUND = 4 x EMUL (test_f32_conditioning's rule: a plain statement stays
within a quarter of the bound; the kernel adds hardware exp2 / log2, another accumulation order and
the forward's f32 lse on top). test_bwd_measure_catches_mutations (CPU) shows the bound is not
loose: the emulation with one thing wrong exceeds it on the sequences of two or more keys of the
named case.

Bit-exact claims (torch.equal), each read from the code: test_bwd_exact_claims."""
import pytest
import torch

import _attn_bwd as G
import _attn_cases as A

DEV = "cuda:0"
gpu_test = pytest.mark.gpu  # per test: the conditioning and mutation tests run without a device

EMUL_BF16, EMUL_F32 = 4.9e-3, 1.9e-6          # measured on the CPU (module docstring)
EMUL_BF16_ONE_KEY, EMUL_F32_ONE_KEY = 3.2e-3, 1.4e-6
EMUL = {(torch.bfloat16, "keys"): EMUL_BF16, (torch.float32, "keys"): EMUL_F32,
        (torch.bfloat16, "one_key"): EMUL_BF16_ONE_KEY, (torch.float32, "one_key"): EMUL_F32_ONE_KEY}
BOUND = {k: 4 * e for k, e in EMUL.items()}
DTYPES = ["bf16", "f32"]
LAYOUTS = ["padded", "packed"]
SHORT = [("t64", f) for f in A.FAMILIES] + [("t1", "randn")]
LONG = ("t2048", "stairs_up", 2, "bf16")
EXACT_FAMILIES = ["stairs_up", "late_spike"]  # test_bwd_exact_claims, test_bwd_forward_lse
# every (shape, family, H, dtype) a device test launches
DEVICE_CASES = ([("t449", f, 2, dt) for f in A.FAMILIES for dt in DTYPES] + [(s, f, 2, dt) for s, f in SHORT for dt in DTYPES]
                + [("t449", "stairs_up", 3, dt) for dt in DTYPES] + [LONG])


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops  # noqa: F401  (loads the library)

    return DEV


def _check(what, got, ref, mag, c, packed):
    errs = G.slice_err(got, ref, mag, c, packed)
    for cls, (err, at) in errs.items():
        if at is not None or cls == "keys":  # at None: no slice of the class differs at all
            print(f"{what}: {cls} err {err:.3e} at (b, len, h, slice) {at} (bound {BOUND[c.dtype, cls]:g})")
    for cls, (err, at) in errs.items():
        assert err < BOUND[c.dtype, cls], (what, cls, err, at, BOUND[c.dtype, cls])


def _run(gpu, family, shape, H, dtype, layout, kind, lse=None, what=None, **pads):
    """One launch against the cached float64 reference; returns the per-sequence result."""
    packed = layout == "packed"
    c, dO, grad, mag = G.ref_for(family, shape, H, dtype, kind, packed)
    got, raw = G.launch_bwd(c, gpu, packed, dO, lse=lse, **pads)
    stats = "own" if lse is None else lse if isinstance(lse, str) else "fwd"
    _check(what or f"{shape}/{family}/H{H}/{dtype}/{layout}/dO {kind}/lse {stats}", got, grad, mag, c, packed)
    return got, raw


# ---- CPU: what the measure gives for a correct and for a broken implementation ----------------------
def test_bwd_conditioning():
    """CPU only. The float32 emulation of the algorithm (module docstring) on every case of the
    device tests stays at or below the pinned EMUL figures, a quarter of the kernel bounds."""
    worst = {}
    for shape, family, H, dtype in DEVICE_CASES:
        combos = [("padded", "randn")] if shape == "t2048" else [("padded", "randn"), ("packed", "randn")]
        if shape in ("t64", "t1") or (H == 2 and family in EXACT_FAMILIES):  # where the device tests mask dO
            combos.append(("padded", "masked"))
        for layout, kind in combos:
            packed = layout == "packed"
            c, dO, grad, mag = G.ref_for(family, shape, H, dtype, kind, packed)
            for cls, (err, at) in G.slice_err(G.emulate(c, dO, packed), grad, mag, c, packed).items():
                print(f"{shape}/{family}/H{H}/{dtype}/{layout}/dO {kind}: emulation {cls} err {err:.3e} at {at}")
                if err > worst.get((c.dtype, cls), (0.0,))[0]:
                    worst[c.dtype, cls] = (err, shape, family, H, layout, kind, at)
    for k, w in worst.items():
        print(f"worst {k}: {w[0]:.3e} {w[1:]} (pinned {EMUL[k]:g})")
    assert set(worst) == set(EMUL)
    for k, w in worst.items():
        assert w[0] <= EMUL[k], (k, w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutation,family,kind", [("mask_last_key", "late_spike", "masked"),
                                                  ("skip_tile0", "stairs_down", "masked"),
                                                  ("d_zero", "randn", "masked"), ("dk_no_temp", "randn", "masked"),
                                                  ("drop_pad_rows", "randn", "randn")])
def test_bwd_measure_catches_mutations(mutation, family, kind, dtype):
    """CPU only. The emulation with one thing wrong exceeds BOUND on t449 of the named family
    (padded): the last valid key masked (an off-by-one in key < len), the first key tile skipped,
    D = 0, dK without 1 / temperature, and the padded query rows (t >= len) left out of dK / dV
    with a dO that is not zero there."""
    c, dO, grad, mag = G.ref_for(family, "t449", 2, dtype, kind, False)
    good = G.slice_err(G.emulate(c, dO, False), grad, mag, c, False)
    bad = G.slice_err(G.emulate(c, dO, False, mutate=mutation), grad, mag, c, False)
    for cls in G.CLASSES:
        print(f"{mutation}/{family}/{dtype}: {cls} err {bad[cls][0]:.3e} at {bad[cls][1]} "
              f"(unmutated {good[cls][0]:.3e}, bound {BOUND[c.dtype, cls]:g})")
        assert good[cls][0] <= EMUL[c.dtype, cls], (cls, good[cls], EMUL[c.dtype, cls])
    # the sequences of two or more keys alone must show it
    assert bad["keys"][0] > BOUND[c.dtype, "keys"], (mutation, family, dtype, bad)


# ---- device ---------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("stats", ["own", "ref"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_bwd_t449(gpu, family, dtype, layout, stats):
    """T = 449 (8 key tiles, the last of one key; 23 sequences with lengths at every 32 / 64 / 128 /
    256 edge, 0 and 1), dO randn on all rows: the padded query rows feed dK / dV."""
    _run(gpu, family, "t449", 2, dtype, layout, "randn", lse=None if stats == "own" else "ref")


@gpu_test
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", EXACT_FAMILIES)
def test_bwd_forward_lse(gpu, family, dtype, layout):
    """lse written on the device by fs2_attention_ex for the same case (what FFTBlockFn passes):
    within BOUND of the reference, and within BOUND of the own-statistics result in the same
    measure."""
    packed = layout == "packed"
    c, dO, grad, mag = G.ref_for(family, "t449", 2, dtype, "randn", packed)
    _, _, raw = A.launch(c, gpu, packed, 0, lse=True)
    fwd, _ = _run(gpu, family, "t449", 2, dtype, layout, "randn", lse=raw["lse"])
    own, _ = G.launch_bwd(c, gpu, packed, dO)
    _check(f"t449/{family}/{dtype}/{layout}: forward lse against own statistics", fwd, own, mag, c, packed)


@gpu_test
@pytest.mark.parametrize("kind", G.DO_KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,family", SHORT)
def test_bwd_short(gpu, shape, family, dtype, layout, kind):
    """T = 64 (one key tile, lengths 64 .. 0) and T = 1, own statistics and the reference's."""
    _run(gpu, family, shape, 2, dtype, layout, kind)
    _run(gpu, family, shape, 2, dtype, layout, kind, lse="ref")


@gpu_test
def test_bwd_long(gpu):
    """T = 2048 (32 key tiles; training crops at 2000), stairs_up, bf16, padded, reference lse."""
    shape, family, H, dtype = LONG
    _run(gpu, family, shape, H, dtype, "padded", "randn", lse="ref")


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
def test_bwd_three_heads(gpu, dtype):
    _run(gpu, "stairs_up", "t449", 3, dtype, "padded", "randn")
    _run(gpu, "stairs_up", "t449", 3, dtype, "packed", "randn", lse="ref")


@gpu_test
@pytest.mark.parametrize("stats", ["own", "ref"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", EXACT_FAMILIES)
def test_bwd_exact_claims(gpu, family, dtype, stats):
    """Read from the code: no atomics, so two launches agree bit for bit; a query row's dQ is
    dS K with dS = P (dP - D), and dP = D = 0 where dO = 0; the rows of the MFMA tiles are
    lane-local and a query row with dO = 0 adds exact zeros to dK / dV, so the packed layout equals
    the padded one on the valid rows under masked dO; a workgroup without a valid key stores the
    zeros its accumulators were initialised with."""
    lse = None if stats == "own" else "ref"
    c, dO, grad, mag = G.ref_for(family, "t449", 2, dtype, "masked", False)
    C, Dm = 3 * c.H * A.DK, c.H * A.DK
    pad, _ = G.launch_bwd(c, gpu, False, dO, lse=lse)
    pad2, _ = G.launch_bwd(c, gpu, False, dO, lse=lse)
    pk, _ = G.launch_bwd(c, gpu, True, dO, lse=lse)
    pk2, _ = G.launch_bwd(c, gpu, True, dO, lse=lse)
    _check(f"t449/{family}/{dtype}/padded/dO masked/lse {stats}", pad, grad, mag, c, False)
    _check(f"t449/{family}/{dtype}/packed/dO masked/lse {stats}", pk, grad, mag, c, True)
    for b, n in enumerate(c.lens):
        tag = (family, dtype, stats, b, n)
        assert torch.equal(pad[b], pad2[b]) and torch.equal(pk[b], pk2[b]), ("two launches differ", tag)
        assert not bool(pad[b][n:, :Dm].any()), ("dQ of a padded query row not zero under masked dO", tag)
        assert not bool(pad[b][n:, Dm:].any()), ("dK / dV of a key >= len not zero", tag)
        assert torch.equal(pad[b][:n], pk[b]), ("packed != padded on the valid rows", tag)
        if n == 0:
            assert not bool(pad[b].any()), ("a sequence without keys is not all zeros", tag)
    # dO randn on all rows: the keys >= len and the sequences without a key still get zeros
    c, dO, grad, mag = G.ref_for(family, "t449", 2, dtype, "randn", False)
    full, _ = G.launch_bwd(c, gpu, False, dO, lse=lse)
    for b, n in enumerate(c.lens):
        assert not bool(full[b][n:, Dm:C].any()), ("dK / dV of a key >= len not zero", family, dtype, stats, b, n)
        assert n > 0 or not bool(full[b].any()), ("a sequence without keys is not all zeros", b)


@gpu_test
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bwd_leaves_alone(gpu, dtype, layout):
    """Row strides with 64 / 8 / 16 / 24 extra columns on qkv / out / dout / dqkv (NaN in the
    inputs' gaps and, packed, in the qkv rows past cu[B]; the sentinel in dqkv and behind the
    2*B*T*H floats of ws): the dqkv gap columns, the rows past cu[B] and the ws tail still hold the
    sentinel, every element below holds none, and the result equals the contiguous launch's bit
    for bit."""
    packed = layout == "packed"
    got, raw = _run(gpu, "stairs_up", "t449", 2, dtype, layout, "randn", qpad=64, opad=8, dpad=16, gpad=24,
                    what=f"strided/{dtype}/{layout}")
    c, dO, _, _ = G.ref_for("stairs_up", "t449", 2, dtype, "randn", packed)
    C, R, g, ws = 3 * c.H * A.DK, raw["rows"], raw["dqkv"], raw["ws"]
    n_ws = 2 * c.B * c.T * c.H
    assert R == (sum(c.lens) if packed else c.B * c.T)
    assert bool(A.is_sentinel(g[:, C:]).all()), "dqkv gap columns written"
    assert bool(A.is_sentinel(g[R:]).all()), "dqkv rows past cu[B] written"
    assert ws.numel() == n_ws + G.WS_TAIL and bool(A.is_sentinel(ws[n_ws:]).all()), "ws written past 2*B*T*H floats"
    assert not bool(A.is_sentinel(g[:R, :C]).any()), "a dqkv element below cu[B] / B*T was left unwritten"
    plain, raw0 = G.launch_bwd(c, gpu, packed, dO)
    assert bool(A.is_sentinel(raw0["dqkv"][R:]).all()) and bool(A.is_sentinel(raw0["ws"][n_ws:]).all())
    assert all(torch.equal(a, b) for a, b in zip(got, plain)), "strided != contiguous"


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
def test_bwd_rejects(gpu, dtype):
    """Every argument error is FS2_EINVAL (an unknown dtype FS2_EUNSUPPORTED) before any launch:
    dqkv and ws still hold the sentinel everywhere. All buffers are valid and in bounds."""
    from fs2amd import _lib as L

    c, dO, _, _ = G.ref_for("randn", "t64", 2, dtype, "randn", False)
    bufs = G.bwd_buffers(c, gpu, False, dO, qpad=16, opad=16, dpad=16, gpad=16)
    cu = A.cu_of(c.lens).to(gpu)
    C, Dm = 3 * c.H * A.DK, c.H * A.DK
    odd = 4 if dtype == "bf16" else 2  # a multiple of 4 (2) elements, not of 8 (4)
    bad = {"both key_lens and seq_cu": dict(seq_cu=cu), "neither key_lens nor seq_cu": dict(key_lens=None),
           "dk 64": dict(dk=64), "dk 256": dict(dk=256), "temperature 0": dict(temperature=0.0),
           "temperature < 0": dict(temperature=-1.0), "qkv stride below 3*H*dk": dict(qkv_row_stride=C - 8),
           "out stride below H*dk": dict(out_row_stride=Dm - 8), "dout stride below H*dk": dict(dout_row_stride=Dm - 8),
           "dqkv stride below 3*H*dk": dict(dqkv_row_stride=C - 8), "qkv stride odd": dict(qkv_row_stride=C + odd),
           "out stride odd": dict(out_row_stride=Dm + odd), "dout stride odd": dict(dout_row_stride=Dm + 2),
           "dqkv stride odd": dict(dqkv_row_stride=C + 2), "ws one float short": dict(ws_bytes=2 * c.B * c.T * c.H * 4 - 4)}
    for what, over in bad.items():
        assert G.call_bwd(c, bufs, **over) == L.FS2_EINVAL, what
    assert G.call_bwd(c, bufs, dtype=7) == L.FS2_EUNSUPPORTED
    assert G.call_bwd(c, bufs, dtype=L.FS2_FP8) == L.FS2_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(A.is_sentinel(bufs["dqkv"]).all()) and bool(A.is_sentinel(bufs["ws"]).all()), "a rejected call launched"
    assert G.call_bwd(c, bufs) == L.FS2_OK  # the same buffers, nothing replaced: accepted
    torch.cuda.synchronize()
    assert not bool(A.is_sentinel(bufs["dqkv"][:, :C]).any())
