"""fs2_attention_ex, every reachable kernel form, on scores that exercise what a flash-style kernel
gets wrong: the online-softmax rescale (attn32_kernel's lazy running max, threshold 8 in the log2
domain = 5.545 nats), p > 1 between rescales, underflow, the key-split merge with range maxima far
apart, tile edges and the ring wrap, other strides, and what the kernel must leave alone.

Called through the ctypes handle (tests/_attn_cases.py: launch), so the test chooses waves,
strides, lse, seq_cu and split_ws itself. Reference: the plain float64 CPU statement of
transformer/Modules.py:14-25 per sequence and head on the tensors after rounding to the kernel's
dtype. Every case's score property is asserted on the CPU before it is launched
(_attn_cases.check_family).

Bounds. Output: the project's own, 2e-2 (bf16) and 2e-5 (f32) of max|ref| OF THAT SEQUENCE (a
short sequence is not hidden behind a long one); the key-split form 2e-2 as in
test_gpu_ops.py::test_attention_key_split. test_f32_conditioning (CPU) shows the f32 bound is
meaningful for these inputs: a float32 torch statement of the op stays within a quarter of it
(measured: at most 1.5e-6 against 5e-6). The rising families put each sequence's top step at 0
nats for that reason (with the top at +68 nats the f32 statement itself was off by 1.3e-5).
lse has no project number: max |lse_f32cpu - lse_f64| over the f32 cases measured 1.29e-5 log2
units on the CPU (late_spike, T = 449), pinned below as LSE_F32CPU = 1.3e-5, and the bound is
16 x that, LSE_BOUND = 2.08e-4 log2 units (the kernel adds hardware exp2 / log2 and an f32
m * scale + log2(l) on top of f32 accumulation). lse is +inf exactly where a sequence has no key.

Bit-exact claims (torch.equal) on the adversarial families: waves 4 = waves 8; split = unsplit for
sequences of <= 256 keys; split repeatable and independent of the T bucket; packed = padded on the
valid rows with padded query rows whose own running max trips the threshold (the last partial
wave's neighbours then differ between the layouts: while every lane of a wave took the new maximum
whenever ANY lane's tripped, the bf16 forms failed this for most sequences with a partial last
wave; the rescale is lane-local in effect now)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import _attn_cases as A

DEV = "cuda:0"
gpu_test = pytest.mark.gpu  # per test: test_f32_conditioning runs without a device

FORMS = {"bf16w4": ("bf16", 4), "bf16w8": ("bf16", 8), "f32": ("f32", 0)}
BOUND = {torch.bfloat16: 2e-2, torch.float32: 2e-5}
LSE_F32CPU = 1.3e-5           # measured on the CPU (module docstring), checked by test_f32_conditioning
LSE_BOUND = 16 * LSE_F32CPU   # log2 units
SHORT = [("t64", "randn"), ("t64", "late_spike"), ("t64", "mixed_wave"), ("t1", "randn")]
F32_CASES = [("t449", f, 2) for f in A.FAMILIES] + [("t449", "stairs_up", 3)] + [(s, f, 2) for s, f in SHORT]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from fs2amd import ops  # noqa: F401  (loads the library)

    return DEV


def _check(c, out, lse, packed, what, bound=None):
    bound = BOUND[c.dtype] if bound is None else bound
    err, at = A.seq_rel_err(out, c.ref, c.lens, c.T, packed)
    print(f"{what}: out err {err:.3e} at (b, len) {at} (bound {bound:g})")
    le = None
    if lse is not None:
        le = A.lse_err(lse, c.lse, c.lens, c.T, packed)
        print(f"{what}: lse err {le:.3e} log2 units (bound {LSE_BOUND:g})")
    assert err < bound, (what, err, at)
    assert le is None or le < LSE_BOUND, (what, le)


def test_f32_conditioning():
    """CPU only. For every f32 case a float32 torch statement of the op stays within a quarter of
    the f32 output bound of the float64 reference, and its lse within LSE_F32CPU (the measured
    figure the lse bound is 16 x of)."""
    worst = 0.0
    for shape, family, H in F32_CASES:
        c = A.make_case(family, shape, H, "f32")
        o32, l32, _ = A.attn_cpu(c.qkv, c.lens, H, c.temperature, torch.float32)
        err, at = A.seq_rel_err(list(o32), c.ref, c.lens, c.T, False)
        le = A.lse_err(list(l32), c.lse, c.lens, c.T, False)
        print(f"{shape}/{family}/H{H}: f32 cpu out err {err:.3e} at {at}, lse err {le:.3e}")
        assert err < 0.25 * BOUND[torch.float32], (shape, family, H, err, at)
        worst = max(worst, le)
    assert worst <= LSE_F32CPU, worst


@gpu_test
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("family", A.FAMILIES)
def test_t449(gpu, family, form, layout):
    """T = 449 (8 key tiles, the last of one key; lengths at every 32 / 64 / 128 / 256 edge, 0 and
    1): attn32_kernel<4,2>, <8,2> and attn_kernel<F32>, with and without lse."""
    dtype, waves = FORMS[form]
    c = A.make_case(family, "t449", 2, dtype)
    packed = layout == "packed"
    out, _, _ = A.launch(c, gpu, packed, waves)
    _check(c, out, None, packed, f"{family}/{form}/{layout}")
    out2, lse, _ = A.launch(c, gpu, packed, waves, lse=True)
    _check(c, out2, lse, packed, f"{family}/{form}/{layout}/lse")


@gpu_test
@pytest.mark.parametrize("form", ["bf16w4", "f32"])
def test_three_heads(gpu, form):
    dtype, waves = FORMS[form]
    c = A.make_case("stairs_up", "t449", 3, dtype)
    out, lse, _ = A.launch(c, gpu, False, waves, lse=True)
    _check(c, out, lse, False, f"stairs_up/H3/{form}")


@gpu_test
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape,family", SHORT)
def test_short(gpu, shape, family, dtype, layout):
    """T <= 64: attn_bf16_kernel<4,2> (one key tile, lengths 64 .. 0) and the f32 kernel; T = 1."""
    c = A.make_case(family, shape, 2, dtype)
    packed = layout == "packed"
    out, lse, _ = A.launch(c, gpu, packed, 0, lse=True)
    _check(c, out, lse, packed, f"{shape}/{family}/{dtype}/{layout}")
    out2, _, _ = A.launch(c, gpu, packed, 0)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


@gpu_test
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("family", A.FAMILIES[1:])
def test_waves_4_equals_8(gpu, family, layout):
    c = A.make_case(family, "t449", 2, "bf16")
    packed = layout == "packed"
    o4, l4, _ = A.launch(c, gpu, packed, 4, lse=True)
    o8, l8, _ = A.launch(c, gpu, packed, 8, lse=True)
    for b in range(c.B):
        assert torch.equal(o4[b], o8[b]) and torch.equal(l4[b], l8[b]), (family, layout, b, c.lens[b])


def _neighbour_events(c):
    """Tiles at which, in the last partial wave of a sequence, a padded query row's running max
    trips the lazy threshold while no valid row's does and a valid row's maximum moves by less
    than the threshold (float64 replay, lane-local): where a wave-wide rescale decision would
    change a valid lane's arithmetic in the padded layout only."""
    n_ev = 0
    for (b, h), st in c.stats.items():
        n, tm = c.lens[b], st["tm"]
        lo, hi = 32 * (n // 32), min(32 * (n // 32) + 32, c.T)
        if n % 32 == 0 or hi <= n or tm.shape[1] < 2:
            continue
        m = tm[lo:hi, 0].clone()
        for t in range(1, tm.shape[1]):
            d = tm[lo:hi, t] - m
            over = d > A.LAZY_NATS
            valid = torch.arange(lo, hi) < n
            if bool(over[~valid].any()) and not bool(over[valid].any()) and bool(((d > 1e-3) & valid).any()):
                n_ev += 1
            m = torch.where(over, tm[lo:hi, t], m)
    return n_ev


@gpu_test
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("family", ["mixed_wave", "late_spike"])
def test_packed_equals_padded_peaked(gpu, family, form):
    """Each query's arithmetic depends on its own keys only (fs2hip.h): the valid rows of the
    padded layout, whose last partial wave holds padded query rows that trip the lazy threshold,
    equal the packed layout's (zero-Q neighbours there) bit for bit."""
    dtype, waves = FORMS[form]
    c = A.make_case(family, "t449", 2, dtype, pad_trip=True)
    assert _neighbour_events(c) >= 4, "the case does not reach a neighbour-driven rescale"
    pad, lpad, _ = A.launch(c, gpu, False, waves, lse=True)
    pk, lpk, _ = A.launch(c, gpu, True, waves, lse=True)
    _check(c, pk, lpk, True, f"{family}/{form}/pad_trip/packed")
    bad = [(b, n) for b, n in enumerate(c.lens)
           if not (torch.equal(pad[b][:n], pk[b]) and torch.equal(lpad[b][:n], lpk[b]))]
    assert not bad, (family, form, "packed != padded on the valid rows of (b, len)", bad)


@gpu_test
@pytest.mark.parametrize("family", ["randn", "stairs_up", "late_spike"])
def test_key_split(gpu, family):
    """T = 2048 packed: the key-split form (256-key ranges merged by the last to arrive; stairs_up
    puts the range maxima 8.5 nats apart) and the SAME input unsplit with waves 4 (attn32_kernel
    <4,2> over up to 32 key tiles), both against the reference for every length; the split form's
    bit-exact claims."""
    c = A.make_case(family, "t2048", 2, "bf16")
    rows = sum(c.lens)
    split, _, _ = A.launch(c, gpu, True, 4, split=rows)
    _check(c, split, None, True, f"{family}/split", bound=2e-2)
    plain, _, _ = A.launch(c, gpu, True, 4)
    _check(c, plain, None, True, f"{family}/unsplit w4")
    again, _, _ = A.launch(c, gpu, True, 4, split=rows)
    T2 = 1536
    lens2 = [min(n, T2) for n in c.lens]
    other, _, _ = A.launch(c, gpu, True, 4, split=sum(lens2), lens=lens2, T=T2)
    for b, n in enumerate(c.lens):
        if n <= 256:
            assert torch.equal(split[b], plain[b]), ("split != unsplit", b, n)
        assert torch.equal(again[b], split[b]), ("nondeterministic", b, n)
        if n <= T2:
            assert torch.equal(other[b], split[b]), ("T-dependent", b, n)
    if family == "stairs_up":  # rows_max = B * T: the largest the header allows
        full, _, _ = A.launch(c, gpu, True, 4, split=c.B * c.T)
        assert all(torch.equal(a, b) for a, b in zip(full, split))


@gpu_test
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("form", list(FORMS))
def test_strides_and_sentinels(gpu, form, layout):
    """qkv_row_stride = 3*H*dk + 64 with NaN in the gap columns, out_row_stride = H*dk + 64, out
    and lse pre-filled with a NaN bit pattern, packed rows past cu[B] NaN in qkv: the gap columns
    and the rows past cu[B] still hold the pattern, every row below holds none and is finite."""
    dtype, waves = FORMS[form]
    c = A.make_case("stairs_up", "t449", 2, dtype)
    packed = layout == "packed"
    out, lse, raw = A.launch(c, gpu, packed, waves, lse=True, qpad=64, opad=64)
    _check(c, out, lse, packed, f"strided/{form}/{layout}")
    D, R = c.H * A.DK, raw["rows"]
    o, l = raw["out"], raw["lse"]
    assert bool(A.is_sentinel(o[:, D:]).all()), "out gap columns written"
    assert bool(A.is_sentinel(o[R:]).all()) and bool(A.is_sentinel(l[R:]).all()), "rows past cu[B] written"
    assert not bool(A.is_sentinel(o[:R, :D]).any()) and bool(torch.isfinite(o[:R, :D].float()).all())
    assert not bool(A.is_sentinel(l[:R]).any()) and not bool(torch.isnan(l[:R]).any())


@gpu_test
@pytest.mark.parametrize("setting", ["FS2_ATTN32=0", "FS2_ATTN32_FORM=8x3"])
def test_env_only_forms(gpu, setting):
    """attn_bf16_kernel<8,2> (FS2_ATTN32=0) and attn32_kernel<8,3> (FS2_ATTN32_FORM=8x3): the
    switches are read once per process, so each runs the T = 449 bf16 table in a fresh child."""
    name, value = setting.split("=")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_forms_child.py")
    r = subprocess.run([sys.executable, child], env=dict(os.environ, **{name: value}), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (setting, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 2 * len(A.FAMILIES)
    for case, e in res.items():
        print(f"{setting} {case}: out err {e['err']:.3e} at {e['at']}, lse err {e['lse']:.3e}")
    for case, e in res.items():
        assert e["err"] < BOUND[torch.bfloat16], (setting, case, e)
        assert e["lse"] < LSE_BOUND, (setting, case, e)
