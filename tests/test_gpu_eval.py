"""Objective evaluation on the GPU (include/fs2hip_eval.h: ops.mel_cepstrum, ops.pair_dist, ops.dtw,
ops.path_stats, fs2amd.evaluate) against the numpy restatements of tests/_eval.py and the values stored
in tests/golden/eval_a.npz.

The cepstrum, the squared distances, the DTW given its costs and the path statistics are determined
bit for bit and compared so. The distance itself goes through the device's float64 square root: it is
held within 1 ulp of numpy's, and the DTW is compared bit for bit against the recursion restated over
the GPU's own costs (which isolates the programme from the square root) and, with u = 2^-52, within
rtol 2 (Tx_b + Ty_b) u of the pure-host restatement: one rounding per path step plus one ulp per cost,
doubled."""
import importlib

import numpy as np
import pytest
import torch

import _eval as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -52
B = len(E.CASES)
X_LENS = [Tx for Tx, _ in E.CASES]
Y_LENS = [Ty for _, Ty in E.CASES]
P = E.TX_MAX + E.TY_MAX - 1
DTYPES = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def fx():
    return E.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def run_dtw(x, x_lens, y, y_lens, **kw):
    from fs2amd import ops

    o = ops.dtw(x if torch.is_tensor(x) else dev(x), x_lens, y if torch.is_tensor(y) else dev(y), y_lens, **kw)
    return o.total.cpu().numpy(), o.K.cpu().numpy(), o.path_i.cpu().numpy(), o.path_j.cpu().numpy()


def run_cost(x, x_lens, y, y_lens, **kw):
    from fs2amd import ops

    return ops.pair_dist(x if torch.is_tensor(x) else dev(x), x_lens, y if torch.is_tensor(y) else dev(y), y_lens,
                         **kw).cpu().numpy()


def expected_over(cost, x_lens, y_lens, width):
    """The recursion restated over a cost tensor [B, Tx_max, Ty_max]: (total, K, path_i, path_j) as the
    kernel lays them out."""
    n = len(x_lens)
    total, K = np.zeros(n), np.zeros(n, dtype=np.int32)
    pi, pj = np.full((n, width), -1, dtype=np.int32), np.full((n, width), -1, dtype=np.int32)
    for b, (Tx, Ty) in enumerate(zip(x_lens, y_lens)):
        total[b], K[b], i, j = E.dtw_from_cost(cost[b, :Tx, :Ty])
        pi[b], pj[b] = E.padded_path(K[b], i, j, width)
    return total, K, pi, pj


def assert_same_dtw(got, want):
    same_bits(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, w)


@pytest.fixture(scope="module")
def runs():
    """The ragged batch once per dtype: the GPU's costs, the recursion restated over them, and ops.dtw
    per bitmap form."""
    out = {}
    for d, dt in DTYPES.items():
        x, y, _, _ = E.batch_feats(dt)
        xd, yd = dev(x), dev(y)
        cost = run_cost(xd, X_LENS, yd, Y_LENS)
        out[d] = {"cost": cost, "want": expected_over(cost, X_LENS, Y_LENS, P),
                  "lds": run_dtw(xd, X_LENS, yd, Y_LENS, bitmap="lds"),
                  "global": run_dtw(xd, X_LENS, yd, Y_LENS, bitmap="global")}
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mel_cepstrum_equals_the_restatement_exactly(dtype):
    from fs2amd import ops

    ev = importlib.import_module("fs2amd.evaluate")
    lens = [40, 17, 1, 33]
    mel = np.full((4, 40, E.N_MEL), np.nan, dtype=DTYPES[dtype])
    for b, T in enumerate(lens):
        mel[b, :T] = E.make_mel(T, 60 + b).astype(DTYPES[dtype])
    basis = E.dct_basis()
    got = ops.mel_cepstrum(dev(mel), lens, basis=dev(basis)).cpu().numpy()
    assert got.shape == (4, 40, E.N_COEF) and got.dtype == np.float64
    for b, T in enumerate(lens):
        same_bits(got[b, :T], E.mel_cepstrum_ref(mel[b, :T], basis))
        assert not got[b, T:].any() and not np.signbit(got[b, T:]).any()
    same_bits(ev.mel_cepstrum(dev(mel), torch.tensor(lens, device=DEV)).cpu().numpy(), got)
    wide = ops.mel_cepstrum(dev(mel), lens, basis=dev(E.dct_basis(E.N_MEL, 30))).cpu().numpy()  # another C
    same_bits(wide[0, :, :E.N_COEF], got[0])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pair_dist_against_numpy(runs, dtype):
    """s bit for bit; the distance within 1 ulp of np.sqrt(s); zeros outside [Tx_b, Ty_b]. Whether the
    device's square root came out correctly rounded everywhere is printed (DESIGN 9.6 records it)."""
    x, y, xs, ys = E.batch_feats(DTYPES[dtype])
    sq = run_cost(x, X_LENS, y, Y_LENS, squared=True)
    cost = runs[dtype]["cost"]
    assert cost.shape == sq.shape == (B, E.TX_MAX, E.TY_MAX) and cost.dtype == np.float64
    n_cells = n_off = 0
    for b, (Tx, Ty) in enumerate(E.CASES):
        s = E.pair_sq_ref(xs[b], ys[b])
        same_bits(sq[b, :Tx, :Ty], s)
        off = np.abs(bits(cost[b, :Tx, :Ty]).astype(np.int64) - bits(np.sqrt(s)).astype(np.int64))
        assert off.max() <= 1, (b, off.max())
        n_cells, n_off = n_cells + off.size, n_off + int((off != 0).sum())
        for a in (sq[b], cost[b]):
            assert not a[Tx:].any() and not a[:, Ty:].any()
    print(f"pair_dist {dtype}: {n_off} of {n_cells} square roots differ from numpy's (by 1 ulp)")


@pytest.mark.parametrize("bitmap", ["lds", "global"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_dtw_equals_the_recursion_over_the_gpu_costs_exactly(runs, dtype, bitmap):
    got, want = runs[dtype][bitmap], runs[dtype]["want"]
    assert got[0].dtype == np.float64 and got[2].shape == got[3].shape == (B, P)
    assert_same_dtw(got, want)
    for b, (Tx, Ty) in enumerate(E.CASES):
        assert max(Tx, Ty) <= got[1][b] <= Tx + Ty - 1


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_dtw_against_the_pure_host_fixture(fx, runs, dtype):
    tag = "32" if dtype == "f32" else ""
    sep = "_" if tag else ""
    total, K, pi, pj = runs[dtype]["lds"]
    np.testing.assert_array_equal(K, fx[f"K{tag}"])
    for b, (Tx, Ty) in enumerate(E.CASES):
        want = fx[f"total{tag}"][b]
        assert abs(total[b] - want) <= 2 * (Tx + Ty) * U * want, (b, total[b], want)
        np.testing.assert_array_equal(pi[b, :K[b]], fx[f"pi{tag}{sep}{b}"])
        np.testing.assert_array_equal(pj[b, :K[b]], fx[f"pj{tag}{sep}{b}"])


def test_dtw_tie_rule_in_the_callers_i_and_j():
    def path(x, y, **kw):
        x = np.asarray(x, dtype=np.float64)[None, :, None]
        y = np.asarray(y, dtype=np.float64)[None, :, None]
        total, K, pi, pj = run_dtw(x, None, y, None, **kw)
        return float(total[0]), list(zip(pi[0, :K[0]].tolist(), pj[0, :K[0]].tolist()))

    for bm in ("lds", "global"):
        assert path([2.0] * 5, [2.0] * 3, bitmap=bm) == (0.0, [(0, 0), (1, 0), (2, 0), (3, 1), (4, 2)])
        assert path([2.0] * 3, [2.0] * 5, bitmap=bm) == (0.0, [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)])
        assert path([0, 3, 7, 7, 12], [1, 7, 13], bitmap=bm) == (4.0, [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)])


def test_dtw_larger_shapes_in_lds_and_in_the_workspace():
    """(524, 520), the LDS nearly full, with a short utterance in the same launch, both bitmaps; (2000,
    700), which the helper sends to the workspace and to the large LDS form; D = 80 over raw mels."""
    from fs2amd import _lib

    shapes = ((524, 520), (300, 10))
    assert _lib.dtw_form(524, 520) == (_lib.FS2_OK, _lib.DTW_LDS)
    x = np.full((2, 524, E.D), np.nan, dtype=np.float32)
    y = np.full((2, 520, E.D), np.nan, dtype=np.float32)
    for b, (Tx, Ty) in enumerate(shapes):
        x[b, :Tx], y[b, :Ty] = E.make_feats(Tx, E.D, 500 + b), E.make_feats(Ty, E.D, 510 + b)
    lens = [s[0] for s in shapes], [s[1] for s in shapes]
    want = expected_over(run_cost(x, lens[0], y, lens[1]), lens[0], lens[1], 524 + 520 - 1)
    for bm in ("lds", "global"):
        assert_same_dtw(run_dtw(x, lens[0], y, lens[1], bitmap=bm), want)

    assert _lib.dtw_form(2000, 700) == (_lib.FS2_OK, _lib.DTW_GLOBAL)
    assert _lib.dtw_lds_bytes(2000, 700, False) > _lib.DTW_LDS_SMALL
    x, y = E.make_feats(2000, E.D, 520)[None], E.make_feats(700, E.D, 521)[None]
    want = expected_over(run_cost(x, None, y, None), [2000], [700], 2699)
    assert_same_dtw(run_dtw(x, None, y, None), want)

    x, y = E.make_mel(150, 530)[None].astype(np.float32), E.make_mel(140, 531)[None].astype(np.float32)
    want = expected_over(run_cost(x, None, y, None), [150], [140], 289)
    for bm in ("lds", "global"):
        assert_same_dtw(run_dtw(x, None, y, None, bitmap=bm), want)


def test_dtw_result_does_not_depend_on_the_batch(runs):
    x, y, xs, ys = E.batch_feats(np.float64)
    base = runs["f64"]["lds"]
    rev = list(range(B))[::-1]
    got = run_dtw(x[rev], [X_LENS[b] for b in rev], y[rev], [Y_LENS[b] for b in rev])
    assert_same_dtw(tuple(g[::-1] for g in got), base)
    for b in (4, 7, 8):  # alone, at its own size; then in another row of a wider, taller, NaN-filled tensor
        Tx, Ty = E.CASES[b]
        total, K, pi, pj = run_dtw(xs[b][None], [Tx], ys[b][None], [Ty])
        same_bits(total[0], base[0][b])
        assert K[0] == base[1][b]
        np.testing.assert_array_equal(pi[0, :K[0]], base[2][b, :K[0]])
        np.testing.assert_array_equal(pj[0, :K[0]], base[3][b, :K[0]])
        bx = torch.full((3, Tx + 5, E.D + 9), float("nan"), dtype=torch.float64, device=DEV)
        by = torch.full((3, Ty + 4, E.D + 3), float("nan"), dtype=torch.float64, device=DEV)
        bx[2, :Tx, :E.D], by[2, :Ty, :E.D] = dev(xs[b]), dev(ys[b])
        vx, vy = bx[:, :Tx + 2, :E.D], by[:, :Ty + 1, :E.D]
        assert not vx.is_contiguous() and vx.stride(2) == 1 and not vy.is_contiguous()
        for bm in ("lds", "global"):
            total, K, pi, pj = run_dtw(vx, torch.tensor([0, 0, Tx], device=DEV), vy, torch.tensor([0, 0, Ty], device=DEV),
                                       bitmap=bm)
            same_bits(total[2], base[0][b])
            assert K[2] == base[1][b] and (pi[2, K[2]:] == -1).all() and (pj[2, K[2]:] == -1).all()
            np.testing.assert_array_equal(pi[2, :K[2]], base[2][b, :K[2]])
            np.testing.assert_array_equal(pj[2, :K[2]], base[3][b, :K[2]])
            assert (total[:2] == np.inf).all() and not K[:2].any() and (pi[:2] == -1).all() and (pj[:2] == -1).all()
            cost = run_cost(vx, torch.tensor([0, 0, Tx], device=DEV), vy, torch.tensor([0, 0, Ty], device=DEV))
            same_bits(cost[2, :Tx, :Ty], runs["f64"]["cost"][b, :Tx, :Ty])
            assert not cost[:2].any() and not cost[2, Tx:].any() and not cost[2, :, Ty:].any()


def test_dtw_writes_its_outputs_and_nothing_else(runs):
    """Sentinel-filled buffers with a guard row on either side: every entry of the outputs is written
    (path entries -1 from K_b on), the guards are not."""
    from fs2amd import ops

    x, y, _, _ = E.batch_feats(np.float32)
    xd, yd = dev(x), dev(y)
    want = runs["f32"]["want"]
    for bm in ("lds", "global"):
        total = torch.full((B + 2,), 12345.0, dtype=torch.float64, device=DEV)
        K = torch.full((B + 2,), -7777, dtype=torch.int32, device=DEV)
        pi = torch.full((B + 2, P), -7777, dtype=torch.int32, device=DEV)
        pj = torch.full((B + 2, P), -7777, dtype=torch.int32, device=DEV)
        o = ops.dtw(xd, X_LENS, yd, Y_LENS, bitmap=bm, out=(total[1:B + 1], K[1:B + 1], pi[1:B + 1], pj[1:B + 1]))
        assert o.path_i.data_ptr() == pi[1].data_ptr()
        assert_same_dtw(tuple(t[1:B + 1].cpu().numpy() for t in (total, K, pi, pj)), want)
        for b in range(B):
            k = int(K[1 + b])
            assert bool((pi[1 + b, k:] == -1).all()) and bool((pj[1 + b, k:] == -1).all())
            assert bool((pi[1 + b, :k] >= 0).all()) and bool((pj[1 + b, :k] >= 0).all())
        for t, s in ((total, 12345.0), (K, -7777), (pi, -7777), (pj, -7777)):
            assert bool((t[0] == s).all()) and bool((t[B + 1] == s).all())


def test_dtw_zero_lengths_and_refusals(runs):
    from fs2amd import ops

    x, y, _, _ = E.batch_feats(np.float64)
    xd, yd = dev(x), dev(y)
    x_bad, y_bad = list(X_LENS), list(Y_LENS)
    x_bad[3] = 0
    y_bad[6] = 0
    for xl, yl in ((x_bad, Y_LENS), (X_LENS, y_bad)):
        with pytest.raises(ValueError):
            ops.dtw(xd, xl, yd, yl)
    with pytest.raises(ValueError):
        ops.dtw(xd, [T + 1000 for T in X_LENS], yd, Y_LENS)  # beyond Tx_max
    with pytest.raises(ValueError, match="bytes"):
        ops.dtw(torch.empty(1, 860, 13, device=DEV), None, torch.empty(1, 860, 13, device=DEV), None, bitmap="lds")
    with pytest.raises(ValueError):
        ops.dtw(xd, X_LENS, yd.float(), Y_LENS)  # two dtypes
    with pytest.raises(ValueError):
        ops.dtw(xd, X_LENS, yd, Y_LENS, bitmap="shared")
    base = runs["f64"]["lds"]
    for bm in ("lds", "global"):  # device lengths: no check on the host; +inf, 0, -1
        total, K, pi, pj = run_dtw(xd, torch.tensor(x_bad, device=DEV), yd, torch.tensor(y_bad, device=DEV), bitmap=bm)
        for b in range(B):
            if b in (3, 6):
                assert total[b] == np.inf and K[b] == 0 and (pi[b] == -1).all() and (pj[b] == -1).all()
            else:
                same_bits(total[b], base[0][b])
                assert K[b] == base[1][b]
                np.testing.assert_array_equal(pi[b], base[2][b])
                np.testing.assert_array_equal(pj[b], base[3][b])


def test_path_stats_and_f0_metrics(runs):
    """Counts and sums bit for bit the restatement's along the paths of the ragged batch, with contours
    that have unvoiced stretches; an all-unvoiced contour gives n_both = 0 and NaN, not an error."""
    import fs2amd
    from fs2amd import ops

    total, K, pi, pj = runs["f64"]["lds"]
    f0a, f0b = np.zeros((B, E.TX_MAX)), np.zeros((B, E.TY_MAX))
    for b, (Tx, Ty) in enumerate(E.CASES):
        f0a[b, :Tx], f0b[b, :Ty] = E.make_f0(Tx, 700 + b), E.make_f0(Ty, 750 + b)
    f0a[4] = 0.0  # utterance 4: a has no voiced frame at all
    ta = np.stack([E.f0_tracks(r) for r in f0a])
    tb = np.stack([E.f0_tracks(r) for r in f0b])
    al = ops.DtwOut(dev(total), dev(K), dev(pi), dev(pj))
    st = ops.path_stats(dev(ta), dev(tb), al.path_i, al.path_j, al.K)
    counts, sums = st.counts.cpu().numpy(), st.sums.cpu().numpy()
    assert counts.shape == (B, 2, 4) and counts.dtype == np.int64 and sums.shape == (B, 2, 2)
    want = [E.path_stats_ref(ta[b], tb[b], pi[b], pj[b], int(K[b])) for b in range(B)]
    for b in range(B):
        np.testing.assert_array_equal(counts[b], want[b][0])
        same_bits(sums[b], want[b][1])
        assert counts[b].sum(axis=1).tolist() == [K[b], K[b]]
    assert (counts[:, 0, 0] > 0).sum() >= 6 and (counts[:, 0, 1:].sum(axis=0) > 0).all()  # every kind occurs
    assert counts[4, 0, 0] == 0 and counts[4, 0, 1] == 0

    m = fs2amd.f0_metrics(dev(f0a), dev(f0b), al)
    np.testing.assert_array_equal(m.counts.cpu().numpy(), counts[:, 0])
    n = counts[:, 0, 0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse_hz, rmse_ct = np.sqrt(sums[:, 0, 1] / n), np.sqrt(sums[:, 1, 1] / n)
    # the Hz track is the input itself: one division and one square root apart, a few ulp. The cents
    # track goes through torch's log2 on the device: each value within 2 ulp of 1200 log2(800) < 12000,
    # 3.7e-12, so a difference within 7.3e-12 and the RMSE with it
    np.testing.assert_allclose(m.rmse_hz.cpu().numpy(), rmse_hz, rtol=4 * U, atol=0, equal_nan=True)
    np.testing.assert_allclose(m.rmse_cents.cpu().numpy(), rmse_ct, rtol=4 * U, atol=1e-11, equal_nan=True)
    assert np.isnan(m.rmse_hz.cpu().numpy()[4]) and np.isnan(m.rmse_cents.cpu().numpy()[4])
    assert np.isfinite(np.delete(m.rmse_hz.cpu().numpy(), 4)).sum() >= 6
    vde = (counts[:, 0, 1] + counts[:, 0, 2]) / K.astype(np.float64)
    np.testing.assert_allclose(m.vde.cpu().numpy(), vde, rtol=2 * U, atol=0)
    assert abs(float(m.pooled_vde) - (counts[:, 0, 1] + counts[:, 0, 2]).sum() / K.sum()) <= 2 * U
    pooled = np.sqrt(sums[:, 0, 1].sum() / n.sum())
    assert abs(float(m.pooled_rmse_hz) - pooled) <= 4 * B * U * pooled and float(m.pooled_rmse_cents) > 0


def test_mcd_identity_stretch_and_fixture(fx, runs):
    import fs2amd

    lens = [37, 12, 1]
    mel = np.full((3, 37, E.N_MEL), np.nan, dtype=np.float32)
    for b, T in enumerate(lens):
        mel[b, :T] = E.make_mel(T, 80 + b)
    m, al = fs2amd.mcd(dev(mel), lens, dev(mel), lens)
    K, pi, pj = al.K.cpu().numpy(), al.path_i.cpu().numpy(), al.path_j.cpu().numpy()
    assert m.dtype == torch.float64 and m.cpu().tolist() == [0.0, 0.0, 0.0] and K.tolist() == lens
    for b, T in enumerate(lens):
        assert pi[b, :T].tolist() == pj[b, :T].tolist() == list(range(T)) and (pi[b, T:] == -1).all()
    # every second frame twice: 0 0 1 2 2 3 4 4 ...
    idx = [np.repeat(np.arange(T), np.where(np.arange(T) % 2 == 0, 2, 1)) for T in lens]
    lens2 = [len(i) for i in idx]
    mel2 = np.full((3, max(lens2), E.N_MEL), np.nan, dtype=np.float32)
    for b, i in enumerate(idx):
        mel2[b, :len(i)] = mel[b, i]
    m, al = fs2amd.mcd(dev(mel), lens, dev(mel2), lens2)
    assert m.cpu().tolist() == [0.0, 0.0, 0.0] and al.K.cpu().tolist() == lens2
    for b, i in enumerate(idx):
        assert al.path_i[b, :len(i)].cpu().tolist() == i.tolist()
        assert al.path_j[b, :len(i)].cpu().tolist() == list(range(len(i)))
    # against other frames: ALPHA * total / K in float64, exactly, over the cepstra's own alignment
    melb = np.full((3, 30, E.N_MEL), np.nan, dtype=np.float32)
    lensb = [30, 19, 4]
    for b, T in enumerate(lensb):
        melb[b, :T] = E.make_mel(T, 90 + b)
    m, al = fs2amd.mcd(dev(mel), lens, dev(melb), lensb)
    ca, cb = fs2amd.mel_cepstrum(dev(mel), lens), fs2amd.mel_cepstrum(dev(melb), lensb)
    al2 = fs2amd.dtw(ca, lens, cb, lensb)
    same_bits(al.total.cpu().numpy(), al2.total.cpu().numpy())
    total, K = al.total.cpu().numpy(), al.K.cpu().numpy()
    same_bits(m.cpu().numpy(), E.ALPHA * total / K.astype(np.float64))
    assert (m.cpu().numpy() > 0).all() and np.isfinite(m.cpu().numpy()).all()
    # and over the fixture batch: the features taken as cepstra
    total, K = runs["f64"]["lds"][:2]
    for b, (Tx, Ty) in enumerate(E.CASES):
        want = E.ALPHA * fx["total"][b] / fx["K"][b]
        got = E.ALPHA * total[b] / np.float64(K[b])
        assert abs(got - want) <= 2 * (Tx + Ty + 2) * U * want


def test_evaluate_losses_and_mcd_over_a_synthetic_corpus(tmp_path):
    import fs2amd
    from _common import configs
    from fs2amd import config as C
    from fs2amd.model import FastSpeech2
    from fs2amd.pipeline import Dataset, to_device, write_synthetic_corpus

    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), 24, seed=0)
    pc, mc, _ = configs()
    pc, tc = dict(pc, path={"preprocessed_path": corpus}), C.ESD_TRAIN_CONFIG
    ds = Dataset("val.txt", pc, mc, tc, sort=True)
    items = [ds[i] for i in range(len(ds))]
    batches = [to_device(b, DEV) for part in (items[:4], items[4:]) for b in ds.collate_fn(part)]
    assert len(batches) >= 2 and len({len(b[0]) for b in batches}) >= 2  # the weights differ
    torch.manual_seed(0)
    model = FastSpeech2(pc, mc).to(DEV).set_precision("fp32")
    loss_fn = fs2amd.FastSpeech2Loss(pc, mc)
    model.eval()
    with torch.no_grad():
        per = [[float(l) for l in loss_fn(b, model(*b[2:]))] for b in batches]
    n = np.array([len(b[0]) for b in batches], dtype=np.float64)
    want = (np.array(per, dtype=np.float64) * n[:, None]).sum(0) / n.sum()
    model.train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ev = importlib.import_module("fs2amd.evaluate")
    out = fs2amd.evaluate(model, batches, pc, mc)
    assert model.training
    after = model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    got = np.array([out[k] for k in ev.LOSS_NAMES])
    print("evaluate:", out)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    assert out["n_utts"] == int(n.sum()) and 1 <= out["n_mcd"] <= out["n_utts"]
    assert np.isfinite(out["mcd"]) and out["mcd"] > 0
    model.eval()
    fs2amd.evaluate(model, batches[:1], pc, mc)
    assert not model.training
