"""Alignment on the GPU (include/fs2hip_align.h: ops.mas, ops.forward_sum, ops.forward_sum_bwd,
fs2amd.align, build_corpus(aligner=...)) against the numpy restatements of tests/_align.py and the
values of torch's CPU float64 ctc_loss stored in tests/golden/align_a.npz.

The search is one add and one comparison per cell: durations, path and score are compared bit for
bit, for float32 and float64 input and for the bitmap in LDS and in global memory. The forward sum
goes through exp and log: with u = 2^-52, nll_b is held to rtol 8 T_b u and the gradient, scaled to
entries in [-1, 1], to atol 16 T_b max(nll_b, 1) u (+ 2^-23 where the output is float32)."""
import filecmp
import os

import numpy as np
import pytest
import torch

import _align as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -52
B = len(A.CASES)
T_LENS = [T for T, _ in A.CASES]
L_LENS = [L for _, L in A.CASES]
DTYPES = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def fx():
    return A.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def run_mas(x, t_lens, l_lens, **kw):
    from fs2amd import ops

    o = ops.mas(x if torch.is_tensor(x) else dev(x), t_lens, l_lens, want_path=True, **kw)
    return o.durations.cpu().numpy(), o.score.cpu().numpy(), o.path.cpu().numpy()


@pytest.fixture(scope="module")
def mas_runs():
    """The ragged batch through ops.mas once per (dtype, bitmap)."""
    return {(d, bm): run_mas(A.batch_logp(DTYPES[d])[0], T_LENS, L_LENS, bitmap=bm)
            for d in DTYPES for bm in ("lds", "global")}


@pytest.fixture(scope="module")
def fs_runs():
    """The ragged batch through ops.forward_sum and ops.forward_sum_bwd once per dtype."""
    from fs2amd import ops

    out = {}
    for d, dt in DTYPES.items():
        x = dev(A.batch_logp(dt)[0])
        o = ops.forward_sum(x, T_LENS, L_LENS, blank_logprob=A.BLANK)
        g = ops.forward_sum_bwd(x, T_LENS, L_LENS, o.alpha, o.nll, None, blank_logprob=A.BLANK)
        out[d] = (float(o.loss.cpu()), o.nll.cpu().numpy(), g.cpu().numpy(), o.alpha.cpu().numpy())
    return out


def expected_mas(fx, tag):
    sep = "_" if tag else ""
    dur = np.zeros((B, A.L_MAX), dtype=np.int64)
    path = np.full((B, A.T_MAX), -1, dtype=np.int32)
    for b, (T, L) in enumerate(A.CASES):
        dur[b, :L] = fx[f"dur{tag}{sep}{b}"]
        path[b, :T] = fx[f"path{tag}{sep}{b}"]
    return dur, fx[f"score{tag}"], path


@pytest.mark.parametrize("bitmap", ["lds", "global"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mas_equals_the_fixture_exactly(fx, mas_runs, dtype, bitmap):
    dur, score, path = mas_runs[(dtype, bitmap)]
    want_dur, want_score, want_path = expected_mas(fx, "32" if dtype == "f32" else "")
    np.testing.assert_array_equal(dur, want_dur)
    np.testing.assert_array_equal(path, want_path)
    same_bits(score, want_score)
    assert dur.dtype == np.int64 and path.dtype == np.int32 and score.dtype == np.float64
    for b, (T, L) in enumerate(A.CASES):
        assert dur[b, :L].min() >= 1 and dur[b].sum() == T


def test_mas_tie_takes_the_diagonal_and_a_built_path_comes_back():
    dur, score, path = run_mas(np.zeros((1, 5, 3), dtype=np.float32), [5], [3])
    assert dur.tolist() == [[3, 1, 1]] and score.tolist() == [0.0] and path.tolist() == [[0, 0, 0, 1, 2]]
    want = [2, 1, 4, 1, 3]
    for bm in ("auto", "global"):
        dur, score, _ = run_mas(A.path_matrix(want, 11, 5)[None], [11], [5], bitmap=bm)
        assert dur.tolist() == [want] and score.tolist() == [0.0]


def test_mas_long_rows_take_the_strided_and_large_forms():
    """L past two chunks of the workgroup (the cells fetched in the loop, not a frame ahead) and a
    bitmap past the small LDS form; the second utterance is short, in the same launch."""
    from fs2amd import _lib

    shapes = ((524, 520), (300, 10))
    assert _lib.mas_lds_bytes(524, 520) > _lib.MAS_LDS_SMALL
    x = np.full((2, 524, 520), np.nan)
    for b, (T, L) in enumerate(shapes):
        x[b, :T, :L] = A.make_logp(T, L, 40 + b)
    for bm in ("lds", "global"):
        dur, score, path = run_mas(x, [s[0] for s in shapes], [s[1] for s in shapes], bitmap=bm)
        for b, (T, L) in enumerate(shapes):
            d, s, p = A.mas_ref(x[b, :T, :L])
            np.testing.assert_array_equal(dur[b, :L], d)
            np.testing.assert_array_equal(path[b, :T], p)
            same_bits(score[b], np.float64(s))
            assert not dur[b, L:].any() and (path[b, T:] == -1).all()


def test_mas_result_does_not_depend_on_the_batch(fx, mas_runs):
    full, mats = A.batch_logp(np.float64)
    base_dur, base_score, base_path = mas_runs[("f64", "lds")]
    rev = list(range(B))[::-1]
    dur, score, path = run_mas(full[rev], [T_LENS[b] for b in rev], [L_LENS[b] for b in rev])
    np.testing.assert_array_equal(dur[::-1], base_dur)
    np.testing.assert_array_equal(path[::-1], base_path)
    same_bits(score[::-1], base_score)
    for b in (4, 6):  # alone, at its own size; then in another row of a wider, taller, NaN-filled tensor
        T, L = A.CASES[b]
        dur, score, path = run_mas(mats[b][None], [T], [L])
        np.testing.assert_array_equal(dur[0], base_dur[b, :L])
        np.testing.assert_array_equal(path[0], base_path[b, :T])
        same_bits(score[0], base_score[b])
        big = torch.full((3, T + 5, L + 9), float("nan"), dtype=torch.float64, device=DEV)
        big[2, :T, :L] = dev(mats[b])
        view = big[:, :T + 2, :L + 1]
        assert not view.is_contiguous() and view.stride(2) == 1
        for bm in ("lds", "global"):
            dur, score, path = run_mas(view, torch.tensor([0, 0, T], device=DEV), torch.tensor([0, 0, L], device=DEV),
                                       bitmap=bm)
            np.testing.assert_array_equal(dur[2, :L], base_dur[b, :L])
            np.testing.assert_array_equal(path[2, :T], base_path[b, :T])
            same_bits(score[2], base_score[b])
            assert not dur[:2].any() and (path[:2] == -1).all() and (score[:2] == -np.inf).all()


def test_mas_writes_its_outputs_and_nothing_else(fx):
    """Sentinel-filled buffers with a guard row on either side: every entry of the outputs is written
    (durations 0 beyond L_b, path -1 beyond T_b), the guards are not."""
    from fs2amd import ops

    x = dev(A.batch_logp(np.float32)[0])
    want_dur, want_score, want_path = expected_mas(fx, "32")
    for bm in ("lds", "global"):
        dur = torch.full((B + 2, A.L_MAX), -7777, dtype=torch.int64, device=DEV)
        score = torch.full((B + 2,), 12345.0, dtype=torch.float64, device=DEV)
        path = torch.full((B + 2, A.T_MAX), -7777, dtype=torch.int32, device=DEV)
        o = ops.mas(x, T_LENS, L_LENS, bitmap=bm, out=(dur[1:B + 1], score[1:B + 1], path[1:B + 1]))
        assert o.durations.data_ptr() == dur[1].data_ptr()
        np.testing.assert_array_equal(dur[1:B + 1].cpu().numpy(), want_dur)
        np.testing.assert_array_equal(path[1:B + 1].cpu().numpy(), want_path)
        same_bits(score[1:B + 1].cpu().numpy(), want_score)
        for t, s in ((dur, -7777), (path, -7777), (score, 12345.0)):
            assert bool((t[0] == s).all()) and bool((t[B + 1] == s).all())


def test_lengths_a_monotonic_path_cannot_fit():
    from fs2amd import ops

    full, _ = A.batch_logp(np.float64)
    x = dev(full)
    t_bad, l_bad = list(T_LENS), list(L_LENS)
    t_bad[3], l_bad[3] = 2, 3  # T_b < L_b
    t_bad[5] = 0               # no frames
    l_bad[1] = 0               # no phonemes
    for t, l in ((t_bad, L_LENS), (T_LENS, l_bad), ([t_bad[b] if b == 3 else T_LENS[b] for b in range(B)],
                                                    [l_bad[b] if b == 3 else L_LENS[b] for b in range(B)])):
        with pytest.raises(ValueError):
            ops.mas(x, t, l)
    with pytest.raises(ValueError):
        ops.mas(x, [T + 1000 for T in T_LENS], L_LENS)  # beyond T_max
    with pytest.raises(ValueError, match="bytes"):
        ops.mas(torch.empty(1, 1281, 1000, device=DEV), bitmap="lds")
    base = run_mas(x, T_LENS, L_LENS)
    skipped = (1, 3, 5)
    for bm in ("lds", "global"):  # device lengths: no check on the host; a zero row, -inf, -1
        dur, score, path = run_mas(x, torch.tensor(t_bad, device=DEV), torch.tensor(l_bad, device=DEV), bitmap=bm)
        for b in range(B):
            if b in skipped:
                assert not dur[b].any() and score[b] == -np.inf and (path[b] == -1).all()
            else:
                np.testing.assert_array_equal(dur[b], base[0][b])
                same_bits(score[b], base[1][b])
                np.testing.assert_array_equal(path[b], base[2][b])
    # the forward sum: contribution 0, a zero gradient, the other rows unchanged
    o0 = ops.forward_sum(x, T_LENS, L_LENS)
    g0 = ops.forward_sum_bwd(x, T_LENS, L_LENS, o0.alpha, o0.nll).cpu().numpy()
    o1 = ops.forward_sum(x, t_bad, l_bad)
    g1 = ops.forward_sum_bwd(x, t_bad, l_bad, o1.alpha, o1.nll).cpu().numpy()
    nll0, nll1 = o0.nll.cpu().numpy(), o1.nll.cpu().numpy()
    keep = [b for b in range(B) if b not in skipped]
    assert np.isinf(nll1[list(skipped)]).all() and (nll1[list(skipped)] > 0).all()
    same_bits(nll1[keep], nll0[keep])
    same_bits(g1[keep], g0[keep])
    assert not g1[list(skipped)].any() and not np.isnan(g1).any()
    want = sum(nll1[b] / l_bad[b] for b in keep) / B
    assert float(o1.loss.cpu()) == want


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_forward_sum_nll_within_the_bound(fx, fs_runs, dtype):
    loss, nll, _, _ = fs_runs[dtype]
    want = fx["nll32" if dtype == "f32" else "nll"]
    worst = 0.0
    for b, (T, L) in enumerate(A.CASES):
        rel = abs(nll[b] - want[b]) / abs(want[b])
        worst = max(worst, rel / (T * U))
        print(f"forward_sum[{dtype}] b={b} T={T} L={L}: nll {nll[b]:.17g} torch {want[b]:.17g} rel err {rel:.3e} "
              f"= {rel / (T * U):.3f} T u (bound 8 T u)")
    print(f"forward_sum[{dtype}]: worst nll error {worst:.3f} T u")
    for b, (T, L) in enumerate(A.CASES):
        assert abs(nll[b] - want[b]) <= 8 * T * U * abs(want[b]), (b, nll[b], want[b])
    acc = 0.0
    for b, L in enumerate(L_LENS):
        acc = acc + nll[b] / L
    assert loss == acc / B  # the same operations in the same order


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_forward_sum_gradient_within_the_bound_and_zero_outside(fx, fs_runs, dtype):
    _, nll, grad, _ = fs_runs[dtype]
    tag = "32_" if dtype == "f32" else ""
    assert grad.dtype == DTYPES[dtype] and grad.shape == (B, A.T_MAX, A.L_MAX)
    worst = 0.0
    errs = []
    for b, (T, L) in enumerate(A.CASES):
        scaled = grad[b, :T, :L].astype(np.float64) * (L * B)
        want = fx[f"grad{tag}{b}"]
        tol = 16 * T * max(fx["nll32" if dtype == "f32" else "nll"][b], 1.0) * U + (2.0 ** -23 if dtype == "f32" else 0.0)
        err = np.abs(scaled - want).max()
        errs.append((b, err, tol))
        worst = max(worst, err / tol)
        print(f"forward_sum_bwd[{dtype}] b={b} T={T} L={L}: max |grad * L B - torch| {err:.3e} (bound {tol:.3e})")
        assert np.abs(want).max() <= 1.0
    print(f"forward_sum_bwd[{dtype}]: worst error {worst:.4f} of its bound")
    for b, err, tol in errs:
        assert err <= tol, (b, err, tol)
    for b, (T, L) in enumerate(A.CASES):  # exact zeros (not -0.0, not NaN) outside the extents
        out = grad[b].copy()
        out[:T, :L] = 0
        assert not bits(out).any(), b


def test_forward_sum_long_rows_against_torch_ctc():
    """More than two chunks of states per workgroup: the labels past the first 512 are fetched in the
    loop. Reference: torch's CPU float64 ctc_loss and autograd, computed here (milliseconds)."""
    import torch.nn.functional as F
    from fs2amd import ops

    shapes = ((524, 520), (300, 10))
    x = np.full((2, 524, 520), np.nan)
    for b, (T, L) in enumerate(shapes):
        x[b, :T, :L] = A.make_logp(T, L, 40 + b)
    t_lens, l_lens = [s[0] for s in shapes], [s[1] for s in shapes]
    xd = dev(x)
    o = ops.forward_sum(xd, t_lens, l_lens)
    grad = ops.forward_sum_bwd(xd, t_lens, l_lens, o.alpha, o.nll).cpu().numpy()
    nll = o.nll.cpu().numpy()
    for b, (T, L) in enumerate(shapes):
        xt = torch.tensor(x[b, :T, :L], requires_grad=True)
        z = torch.cat([torch.full((T, 1), A.BLANK, dtype=torch.float64), xt], dim=1)
        want = F.ctc_loss(F.log_softmax(z, dim=1)[:, None, :], torch.arange(1, L + 1)[None], [T], [L], reduction="sum",
                          zero_infinity=True)
        want.backward()
        want = float(want.detach())
        rel = abs(nll[b] - want) / abs(want)
        err = np.abs(grad[b, :T, :L] * (L * 2) - xt.grad.numpy()).max()
        tol = 16 * T * max(want, 1.0) * U
        print(f"forward_sum long b={b} T={T} L={L}: nll rel err {rel / (T * U):.3f} T u, grad err {err:.3e} (bound {tol:.3e})")
        assert rel <= 8 * T * U and err <= tol
        out = grad[b].copy()
        out[:T, :L] = 0
        assert not bits(out).any()


def test_forward_sum_bwd_writes_its_slab_and_nothing_else(fs_runs):
    from fs2amd import ops

    x = dev(A.batch_logp(np.float64)[0])
    o = ops.forward_sum(x, T_LENS, L_LENS)
    buf = torch.full((B + 2, A.T_MAX, A.L_MAX), 4321.0, dtype=torch.float64, device=DEV)
    g = ops.forward_sum_bwd(x, T_LENS, L_LENS, o.alpha, o.nll, out=buf[1:B + 1])
    assert g.data_ptr() == buf[1].data_ptr()
    same_bits(buf[1:B + 1].cpu().numpy(), fs_runs["f64"][2])
    assert bool((buf[0] == 4321.0).all()) and bool((buf[B + 1] == 4321.0).all())
    # alpha: written inside [T_b, 2 L_b + 1], the same bits from a batch in another order
    rev = list(range(B))[::-1]
    o2 = ops.forward_sum(x[rev], [T_LENS[b] for b in rev], [L_LENS[b] for b in rev])
    same_bits(o2.nll.cpu().numpy()[::-1], fs_runs["f64"][1])
    a1, a2 = fs_runs["f64"][3], o2.alpha.cpu().numpy()[::-1]
    for b, (T, L) in enumerate(A.CASES):
        same_bits(a2[b, :T, :2 * L + 1], a1[b, :T, :2 * L + 1])


def test_autograd_through_the_loss_scales_with_the_upstream_factor(fs_runs):
    import fs2amd
    import fs2amd.library  # noqa: F401  (registers torch.ops.fs2.*)

    full = A.batch_logp(np.float64)[0]
    base = fs_runs["f64"][2]
    crit = fs2amd.ForwardSumLoss(blank_logprob=A.BLANK)
    for how in ("module", "op"):
        x = dev(np.nan_to_num(full, nan=0.0)).requires_grad_(True)  # finite padding: 3.5 * 0 stays 0 upstream
        if how == "module":
            loss = crit(x, T_LENS, L_LENS)
        else:
            loss = torch.ops.fs2.forward_sum(x, torch.tensor(T_LENS, device=DEV), torch.tensor(L_LENS, device=DEV),
                                             A.BLANK)[0]
        assert loss.dtype == torch.float64 and loss.shape == () and float(loss.detach()) == fs_runs["f64"][0]
        (3.5 * loss).backward()
        g = x.grad.cpu().numpy()
        assert g.shape == base.shape and np.abs(g - 3.5 * base).max() <= 4 * U * np.abs(3.5 * base).max()
        for b, (T, L) in enumerate(A.CASES):
            out = g[b].copy()
            out[:T, :L] = 0
            assert not out.any()


def _synthetic_alignment_task(seed=0, n_utts=8, n_symbols=10, n_mel=16):
    """Every phoneme id has its own mel vector; an utterance holds each of its phonemes for 1-5 frames, plus noise."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((n_symbols, n_mel)).astype(np.float32) * 2.0
    ids, mels, durs = [], [], []
    for _ in range(n_utts):
        L = int(rng.integers(3, 9))
        p = rng.integers(0, n_symbols, L)
        d = rng.integers(1, 6, L)
        ids.append(p.astype(np.int64))
        durs.append(d)
        mels.append((np.repeat(proto[p], d, axis=0) + 0.1 * rng.standard_normal((int(d.sum()), n_mel))).astype(np.float32))
    assert max(len(m) for m in mels) <= 40 and max(len(p) for p in ids) <= 8
    return ids, mels, durs


def test_fit_aligner_lowers_the_loss_and_align_gives_valid_durations():
    from fs2amd.align import Aligner, AlignmentEncoder, align, fit_aligner

    torch.manual_seed(0)
    ids, mels, _ = _synthetic_alignment_task()
    enc = AlignmentEncoder(10, n_mel=16, d_text=32, d_att=16, temperature=0.05).to(DEV)
    al = Aligner(enc, {str(i): i for i in range(10)})
    batch = al.pack(ids, mels)
    history = fit_aligner(enc, [batch], steps=40, lr=1e-3)
    print(f"fit_aligner: loss {history[0]:.4f} -> {history[-1]:.4f}")
    assert len(history) == 40 and all(np.isfinite(history)) and history[-1] < history[0]
    got = align(enc, *batch)
    assert len(got) == len(ids)
    for d, p, m in zip(got, ids, mels):
        assert d.dtype == np.int64 and d.shape == p.shape and d.min() >= 1 and d.sum() == len(m)
    for a, b in zip(got, al.durations(ids, mels)):
        np.testing.assert_array_equal(a, b)
    assert enc.training


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_build_corpus_takes_durations_from_an_aligner(tmp_path):
    import fs2amd
    from fs2amd.align import Aligner, AlignmentEncoder
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from fs2amd.pipeline import PINYIN_PHONEMES
    from test_gpu_prep import _utterances

    pc, _, _ = synthetic_configs(str(tmp_path / "cfg"))
    utts = _utterances(np.random.default_rng(5))
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    kw = dict(stft=stft, val_size=2, seed=1234, batch_size=4, emotions=SYNTH_EMOTIONS)
    torch.manual_seed(1)
    symbols = {p: i for i, p in enumerate(PINYIN_PHONEMES)}
    aligner = Aligner(AlignmentEncoder(len(symbols), n_mel=80, d_text=32, d_att=16).to(DEV), symbols)

    # utterances that bring durations: byte-identical with and without an aligner
    a, b = str(tmp_path / "plain"), str(tmp_path / "with_aligner")
    lines = fs2amd.build_corpus(a, utts, pc, **kw)
    assert fs2amd.build_corpus(b, utts, pc, aligner=aligner, **kw) == lines and len(lines) >= 4
    files = _tree(a)
    assert files == _tree(b) and len(files) > 5
    match, mismatch, errors = filecmp.cmpfiles(a, b, files, shallow=False)
    assert not mismatch and not errors and len(match) == len(files), (mismatch, errors)

    # utterances without durations (one keeps its own: a batch may mix both)
    bare = [{k: v for k, v in u.items() if k != "durations" or i == 1} for i, u in enumerate(utts)]
    with pytest.raises(KeyError):
        fs2amd.build_corpus(str(tmp_path / "none"), bare, pc, **kw)
    c = str(tmp_path / "aligned")
    lines = fs2amd.build_corpus(c, bare, pc, aligner=aligner, **kw)
    assert len(lines) >= 4 and os.path.getsize(os.path.join(c, "train.txt")) > 0
    names = {u["basename"]: u for u in utts}
    seen = 0
    for line in lines:
        name, spk = line.split("|")[:2]
        d = np.load(os.path.join(c, "duration", f"{spk}-duration-{name}.npy"))
        mel = np.load(os.path.join(c, "mel", f"{spk}-mel-{name}.npy"))
        u = names[name]
        assert d.dtype == np.int64 and d.shape == (len(u["phones"]),) and d.sum() == mel.shape[0]
        if name == utts[1]["basename"]:
            np.testing.assert_array_equal(d, u["durations"])
        else:
            assert d.min() >= 1 and mel.shape[0] == len(u["wav"]) // 256 + 1  # every frame of the waveform's mel
        seen += 1
    assert seen == len(lines)
