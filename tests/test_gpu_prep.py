"""Corpus preprocessing on the GPU (include/fs2hip_prep.h, fs2amd.preprocess) against the reference's
outputs stored in tests/golden/prep_a.npz and the host restatement of tests/_prep.py.

Exact (bit for bit): the interpolated contour, the voiced count, quartiles, masks, counts, the
normalised values with their minimum and maximum. Bounded: the phoneme means (d * 2^-52 * max|segment|,
a d-term float64 sum on both sides) and the running mean / variance (N * 2^-53 and N * 2^-53 * kappa
against the exact rational values, the bound for updating algorithms)."""
import json
import os
import random

import numpy as np
import pytest
import torch

import _prep as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def fx():
    return P.load_fixture()


@pytest.fixture(scope="module")
def pitch(fx):
    """The fixture's pitch cases with one batched launch over all of them."""
    from fs2amd import ops

    f0s, durs = P.ragged(fx, "f0", "f0_lens"), P.ragged(fx, "dur", "dur_lens")
    f0, frames = pack(f0s, np.float64)
    dur, _ = pack(durs, np.int64)
    o = ops.pitch_targets(dev(f0), dev(dur), torch.from_numpy(frames))
    return {"f0s": f0s, "durs": durs, "filled": P.ragged(fx, "ref_filled", "ref_filled_lens"),
            "ph": P.ragged(fx, "ref_ph", "ref_ph_lens"), "out": o.out.cpu().numpy(), "got_filled": o.filled.cpu().numpy(),
            "voiced": o.voiced.cpu().numpy(), "f0": f0, "dur": dur, "frames": frames}


def pack(arrays, dtype, width=None):
    lens = np.array([len(a) for a in arrays], dtype=np.int64)
    out = np.zeros((len(arrays), width or max(int(lens.max()), 1)), dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out, lens


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(bits(a), bits(b))


def test_filled_contour_and_voiced_count_are_the_reference_bits(fx, pitch):
    from fs2amd import ops

    assert (pitch["voiced"] == fx["ref_voiced"]).all() and pitch["voiced"].dtype == np.int32
    for b, (f0, d) in enumerate(zip(pitch["f0s"], pitch["durs"])):
        got = pitch["got_filled"][b]
        if fx["ref_voiced"][b] <= 1:  # dropped: all-zero rows
            assert (bits(got) == 0).all() and (bits(pitch["out"][b]) == 0).all(), fx["pitch_names"][b]
            continue
        n = min(len(f0), int(d.sum()))
        same_bits(got[:n], pitch["filled"][b])
        assert (bits(got[n:]) == 0).all(), fx["pitch_names"][b]
    # without the contour kept (it is staged in LDS instead) the targets are the same bits
    o = ops.pitch_targets(dev(pitch["f0"]), dev(pitch["dur"]), torch.from_numpy(pitch["frames"]), want_filled=False)
    assert o.filled is None
    same_bits(o.out.cpu().numpy(), pitch["out"])
    assert (o.voiced.cpu().numpy() == fx["ref_voiced"]).all()


def test_phoneme_means_within_the_summation_bound(fx, pitch):
    checked = 0
    for b, d in enumerate(pitch["durs"]):
        got = pitch["out"][b]
        if fx["ref_voiced"][b] <= 1:
            continue
        bound = P.mean_bounds(pitch["filled"][b], d)
        err = np.abs(got[:len(d)] - pitch["ph"][b])
        print(f"{fx['pitch_names'][b]}: max err / bound = {np.max(err[d > 0] / bound[d > 0]):.3f}")
        assert (err <= bound).all(), (fx["pitch_names"][b], err.max())
        assert (bits(got[:len(d)][d == 0]) == 0).all() and (bits(got[len(d):]) == 0).all()
        checked += int((d > 0).sum())
    assert checked >= 100  # phonemes with frames in the six kept cases


def test_pitch_targets_wrapper_drops_what_the_reference_drops(fx, pitch):
    from fs2amd.preprocess import pitch_targets

    res, fil = pitch_targets(pitch["f0s"], pitch["durs"], device=DEV, return_filled=True)
    for b, d in enumerate(pitch["durs"]):
        if fx["ref_voiced"][b] <= 1:
            assert res[b] is None and fil[b] is None
        else:
            same_bits(res[b], pitch["out"][b, :len(d)])
            same_bits(fil[b], pitch["filled"][b])


@pytest.mark.parametrize("tag", ["64", "32"])
def test_outlier_fence_is_numpys_bits(fx, tag):
    from fs2amd import ops
    from fs2amd.preprocess import remove_outlier

    tracks, masks = P.ragged(fx, f"tracks{tag}", "track_lens"), P.ragged(fx, f"mask{tag}", "track_lens")
    vals, lens = pack(tracks, tracks[0].dtype)
    o = ops.outlier_moments(dev(vals), torch.from_numpy(lens))
    q, inl, cnt = o.quartiles.cpu().numpy(), o.inlier.cpu().numpy(), o.count.cpu().numpy()
    assert q.dtype == vals.dtype and inl.dtype == np.bool_ and cnt.dtype == np.int64
    ref_q = fx[f"quart{tag}"]
    assert np.isnan(q[0]).all() and np.isnan(ref_q[0]).all() and cnt[0] == 0  # n = 0
    same_bits(q[1:], ref_q[1:])
    for b, m in enumerate(masks):
        np.testing.assert_array_equal(inl[b, :len(m)], m)
        assert not inl[b, len(m):].any() and cnt[b] == m.sum()
    assert cnt[1] == 0 and lens[1] == 1  # n = 1: no inlier
    mean, m2 = o.mean.cpu().numpy(), o.m2.cpu().numpy()
    for b, (v, m) in enumerate(zip(tracks, masks)):
        if m.sum() == 0:
            assert mean[b] == 0 and m2[b] == 0
        else:
            kept = v[m].astype(np.float64)
            n = len(kept)
            np.testing.assert_allclose(mean[b], kept.mean(), rtol=n * 2.0 ** -52)
            np.testing.assert_allclose(m2[b], ((kept - kept.mean()) ** 2).sum(), rtol=n * 2.0 ** -50)
    if tag == "32":  # the element exactly on the upper fence is out
        v = tracks[-1]
        assert not inl[len(tracks) - 1, :len(v)][v == 12.0].any() and cnt[-1] == len(v) - 1
    for i in (5, 9, len(tracks) - 1):  # the drop-in for one array
        kept = remove_outlier(tracks[i], device=DEV)
        same_bits(kept, tracks[i][masks[i]])


def test_nan_is_never_an_inlier():
    from fs2amd import ops

    v = np.arange(40, dtype=np.float64).reshape(2, 20)
    v[1, 7] = np.nan
    o = ops.outlier_moments(dev(v))
    assert o.inlier[0].all() and not o.inlier[1].any() and o.count.tolist() == [20, 0]
    assert torch.isnan(o.quartiles[1]).all() and not torch.isnan(o.quartiles[0]).any()


def test_scaler_parity_with_the_exact_moments(fx):
    from fs2amd.preprocess import CorpusStats

    for tag in ("64", "32"):
        tracks = P.ragged(fx, f"tracks{tag}", "track_lens")
        stats, ex = CorpusStats(DEV), P.ExactMoments()
        worst = [0.0, 0.0, 0.0, 0.0]
        for i, v in enumerate(tracks):
            stats.partial_fit([v])
            ex.add(v[P.outlier_fence(v)[0]])
            assert stats.n_samples_seen_ == ex.n == fx[f"scaler{tag}_n"][i]
            if ex.n == 0:
                continue
            got = ex.ratios(stats.mean_, stats.var_)
            ref = ex.ratios(fx[f"scaler{tag}_mean"][i], fx[f"scaler{tag}_var"][i])
            worst = [max(a, b) for a, b in zip(worst, got + ref)]
            assert max(got) <= 1.0, (tag, i, got)
            assert max(ref) <= 1.0, (tag, i, ref)
        print(f"scaler{tag}: N = {ex.n}: kernel mean {worst[0]:.3e} var {worst[1]:.3e} of the bound; "
              f"reference mean {worst[2]:.3e} var {worst[3]:.3e}")
        assert stats.scale_ == np.sqrt(stats.var_)
        # one call over the whole list is the same sequence of merges: the same state, bit for bit
        whole = CorpusStats(DEV).partial_fit(tracks)
        assert torch.equal(whole.state, stats.state)
    flat = CorpusStats(DEV).partial_fit([np.full(9, 3.5)])  # zero variance: sklearn's scale_ is 1
    assert flat.n_samples_seen_ == 0 and flat.scale_ == 1.0  # (and a constant track has no inlier at all)


def test_normalize_is_the_reference_bits(fx):
    from fs2amd.preprocess import normalize

    ids = fx["norm_ids"]
    for tag, key, mean, std in (("64", "tracks64", float(fx["scaler64_mean"][-1]), float(fx["scaler64_scale"])),
                                ("32", "tracks32", float(fx["scaler32_mean"][-1]), float(fx["scaler32_scale"])),
                                ("32_off", "tracks32", 0, 1)):
        tracks = [P.ragged(fx, key, "track_lens")[i] for i in ids]
        vals, vmin, vmax = normalize(tracks, mean, std, device=DEV)
        same_bits(np.concatenate(vals), fx[f"norm{tag}"])  # dtype included: float32 stays float32 when off
        assert (vmin, vmax) == tuple(fx[f"norm{tag}_minmax"]), tag


def _views(total_rows, width, stride, dtype, fill):
    """A [total_rows, width] view with row stride `stride` into a buffer filled with `fill`."""
    buf = torch.full((total_rows * stride + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:total_rows * stride].view(total_rows, stride)[:, :width]


def test_an_utterance_gives_the_same_bits_alone_and_in_any_batch(fx, pitch):
    from fs2amd import ops

    b0 = list(fx["pitch_names"]).index("three_passes_T700")
    f0, d = pitch["f0s"][b0], pitch["durs"][b0]
    others = [pitch["f0s"][0], pitch["f0s"][2]]
    odurs = [pitch["durs"][0], pitch["durs"][2]]

    def run_pitch(order, T, stride, Lx):
        f0s, ds = [x[0] for x in order], [x[1] for x in order]
        _, view = _views(len(order), T, stride, torch.float64, float("nan"))
        host, frames = pack(f0s, np.float64, T)
        view.copy_(dev(host))
        dur, _ = pack(ds, np.int64, Lx)
        o = ops.pitch_targets(view, dev(dur), torch.from_numpy(frames))
        return o.out.cpu().numpy(), o.filled.cpu().numpy(), o.voiced.cpu().numpy()

    me = (f0, d)
    alone = run_pitch([me], len(f0), len(f0), len(d))
    first = run_pitch([me, (others[0], odurs[0]), (others[1], odurs[1])], len(f0), len(f0), len(d))
    last = run_pitch([(others[0], odurs[0]), (others[1], odurs[1]), me], 1000, 1031, 80)
    for k, got in ((0, first), (2, last)):
        same_bits(got[0][k, :len(d)], alone[0][0])
        same_bits(got[1][k, :len(f0)], alone[1][0])
        assert got[2][k] == alone[2][0]
    same_bits(alone[1][0], pitch["got_filled"][b0, :len(f0)])

    for tag in ("64", "32"):
        tracks = P.ragged(fx, f"tracks{tag}", "track_lens")
        v = tracks[12]  # 1000 values

        def run_values(order, n_max, stride):
            tdt = torch.float64 if tag == "64" else torch.float32
            _, view = _views(len(order), n_max, stride, tdt, float("nan"))
            host, lens = pack(order, v.dtype, n_max)
            view.copy_(dev(host))
            o = ops.outlier_moments(view, torch.from_numpy(lens))
            out, mm = ops.normalize_minmax(view, torch.from_numpy(lens), mean=191.25, std=37.5)
            return [t.cpu().numpy() for t in (o.quartiles, o.inlier, o.count, o.mean, o.m2, out)]

        alone = run_values([v], 1000, 1000)
        first = run_values([v, tracks[10], tracks[5]], 1000, 1000)
        last = run_values([tracks[10], tracks[5], v], 2049, 2100)
        for k, got in ((0, first), (2, last)):
            same_bits(got[0][k], alone[0][0])
            np.testing.assert_array_equal(got[1][k, :1000], alone[1][0])
            assert got[2][k] == alone[2][0]
            same_bits(got[3][k:k + 1], alone[3])
            same_bits(got[4][k:k + 1], alone[4])
            same_bits(got[5][k, :1000], alone[5][0])


def test_padding_is_zero_and_nothing_outside_the_extents_is_written(fx, pitch):
    from fs2amd import ops

    nan = float("nan")
    f0, dur, frames = pitch["f0"], pitch["dur"], pitch["frames"]
    B, T = f0.shape
    Lx = dur.shape[1] + 5  # padded durations
    durp = np.zeros((B, Lx), dtype=np.int64)
    durp[:, :dur.shape[1]] = dur
    obuf, out = _views(B, Lx, Lx, torch.float64, nan)
    fbuf, filled = _views(B, T, T, torch.float64, nan)
    vbuf = torch.full((B + GUARD,), -7, dtype=torch.int32, device=DEV)
    voiced = vbuf[:B]
    ops.pitch_targets(dev(f0), dev(durp), torch.from_numpy(frames), out=(out, filled, voiced))
    assert torch.isnan(obuf[B * Lx:]).all() and torch.isnan(fbuf[B * T:]).all() and (vbuf[B:] == -7).all()
    assert not torch.isnan(out).any() and not torch.isnan(filled).any()
    same_bits(out.cpu().numpy()[:, :dur.shape[1]], pitch["out"])
    same_bits(filled.cpu().numpy(), pitch["got_filled"])
    assert (bits(out.cpu().numpy()[:, dur.shape[1]:]) == 0).all()
    for b, d in enumerate(pitch["durs"]):
        n = min(int(frames[b]), int(d.sum()))
        assert (bits(filled[b, n:].cpu().numpy()) == 0).all() and (bits(out[b, len(d):].cpu().numpy()) == 0).all()

    for tag, tdt in (("64", torch.float64), ("32", torch.float32)):
        tracks = P.ragged(fx, f"tracks{tag}", "track_lens")[:12]
        vals, lens = pack(tracks, tracks[0].dtype, 140)
        vals[np.arange(140)[None, :] >= lens[:, None]] = np.nan  # what lies past lens is never read into a result
        Bv, n_max = vals.shape
        qbuf, q = _views(Bv, 2, 2, tdt, nan)
        ibuf, inl8 = _views(Bv, n_max, n_max, torch.uint8, 0xAB)
        cbuf = torch.full((Bv + GUARD,), -7, dtype=torch.int64, device=DEV)
        mbuf, m2buf = (torch.full((Bv + GUARD,), nan, dtype=torch.float64, device=DEV) for _ in range(2))
        o = ops.outlier_moments(dev(vals), torch.from_numpy(lens),
                                out=(q, inl8.view(torch.bool), cbuf[:Bv], mbuf[:Bv], m2buf[:Bv]))
        assert torch.isnan(qbuf[Bv * 2:]).all() and (ibuf[Bv * n_max:] == 0xAB).all() and (cbuf[Bv:] == -7).all()
        assert torch.isnan(mbuf[Bv:]).all() and torch.isnan(m2buf[Bv:]).all()
        assert (inl8 <= 1).all() and not torch.isnan(mbuf[:Bv]).any() and not torch.isnan(m2buf[:Bv]).any()
        masks = P.ragged(fx, f"mask{tag}", "track_lens")[:12]
        for b, m in enumerate(masks):
            assert (inl8[b, len(m):] == 0).all() and cbuf[b] == m.sum()
            np.testing.assert_array_equal(inl8[b, :len(m)].cpu().numpy().astype(bool), m)
        same_bits(q.cpu().numpy()[1:], fx[f"quart{tag}"][1:12])
        nbuf, nout = _views(Bv, n_max, n_max, torch.float64, nan)
        mmbuf = torch.full((2 + GUARD,), nan, dtype=torch.float64, device=DEV)
        ops.normalize_minmax(dev(vals), torch.from_numpy(lens), mean=10.0, std=3.0, out=(nout, mmbuf[:2]))
        assert torch.isnan(nbuf[Bv * n_max:]).all() and torch.isnan(mmbuf[2:]).all() and not torch.isnan(nout).any()
        ref, rmin, rmax = P.normalize([t for t in tracks if len(t)], np.float64(10.0), np.float64(3.0))
        assert mmbuf[:2].tolist() == [rmin, rmax]
        for b, t in enumerate(tracks):
            assert (bits(nout[b, len(t):].cpu().numpy()) == 0).all()
            same_bits(nout[b, :len(t)].cpu().numpy(), ((t - np.float64(10.0)) / np.float64(3.0)).astype(np.float64))


def _utterances(rng, n_utts=6):
    from fs2amd.pipeline import PINYIN_PHONEMES

    utts = []
    for u in range(n_utts):
        frames = 30 + 7 * u
        n = 256 * frames  # 1 + n // 256 = frames + 1 frames of mel
        t = np.arange(n) / 22050.0
        wav = (0.4 * np.sin(2 * np.pi * (150.0 + 20 * u) * t) * (0.3 + 0.7 * np.abs(np.sin(3.0 * t + u)))
               + 0.05 * rng.standard_normal(n)).astype(np.float32)
        L = 6 + u
        cuts = np.sort(rng.choice(np.arange(2, frames), size=L - 1, replace=False))
        dur = np.diff(np.concatenate([[0], cuts, [frames]])).astype(np.int64)  # every d >= 1, sum = frames
        if u == 2:  # a zero-length phoneme that is not first
            dur[3] += dur[4]
            dur[4] = 0
        f0 = 170.0 + 10 * u + 30.0 * np.sin(np.arange(frames + 1) / 9.0)
        f0[:2 + u] = 0.0
        f0[12:15] = 0.0
        f0[frames - 3:] = 0.0
        phones = [PINYIN_PHONEMES[j] for j in rng.integers(0, len(PINYIN_PHONEMES), L)]
        utts.append({"basename": f"utt{u:04d}", "speaker": f"spk{u % 3:04d}", "phones": phones, "raw_text": f"raw {u}",
                     "aux": ["Happy|0.5|0.6", "Sad|0.3|0.1", "Angry|0.9|0.2"][u % 3], "wav": wav, "f0": f0,
                     "durations": dur})
    return utts


def test_round_trip_from_waveforms_to_a_forward_pass(tmp_path):
    import fs2amd
    from fs2amd.audio import extract_features
    from fs2amd.config import SYNTH_EMOTIONS, synthetic_configs
    from fs2amd.pipeline import Dataset, to_device
    from fs2amd.preprocess import pitch_targets

    out_dir = str(tmp_path / "corpus")
    pc, mc, tc = synthetic_configs(out_dir)
    utts = _utterances(np.random.default_rng(5))
    stft = fs2amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).to(DEV)
    lines = fs2amd.build_corpus(out_dir, utts, pc, stft=stft, val_size=2, seed=1234, batch_size=4,
                                emotions=SYNTH_EMOTIONS)
    assert len(lines) == 6
    with open(os.path.join(out_dir, "val.txt")) as f:
        val = f.read().splitlines()
    with open(os.path.join(out_dir, "train.txt")) as f:
        train = f.read().splitlines()
    assert val == lines[:2] and train == lines[2:]
    expected = [f"utt{u:04d}" for u in range(6)]
    random.Random(1234).shuffle(expected)
    assert [m.split("|")[0] for m in lines] == expected
    assert lines[0].split("|")[1:3] == [f"spk{int(expected[0][3:]) % 3:04d}", "{" + " ".join(
        utts[int(expected[0][3:])]["phones"]) + "}"]
    assert json.load(open(os.path.join(out_dir, "speakers.json"))) == {"spk0000": 0, "spk0001": 1, "spk0002": 2}

    # stats.json against the host restatement over the same arrays: the phoneme-level pitch and
    # energy tracks as the kernels give them (bit-identical in any batch)
    wav, lens = pack([u["wav"] for u in utts], np.float32)
    feats = extract_features(dev(wav), lens, [u["durations"] for u in utts], stft=stft)
    ph = pitch_targets([u["f0"] for u in utts], [u["durations"] for u in utts], device=DEV)
    for u, p in zip(utts, ph):  # and those are the restatement's means within the summation bound
        r_ph, r_filled, _ = P.pitch_target(u["f0"], u["durations"])
        assert (np.abs(p - r_ph) <= P.mean_bounds(r_filled, u["durations"])).all()
    stats = json.load(open(os.path.join(out_dir, "stats.json")))
    for kind, tracks in (("pitch", ph), ("energy", feats["energy"])):
        ex = P.ExactMoments()
        for v in tracks:
            ex.add(v[P.outlier_fence(v)[0]])
        vmin, vmax, mean, std = stats[kind]
        r_mean, r_var = ex.ratios(mean, std * std)
        print(f"stats.json {kind}: N = {ex.n}, mean {r_mean:.3e} var {r_var:.3e} of the bound")
        # the file holds std = sqrt(var): squaring it back adds two roundings (the root and the
        # square, 2^-53 each, relative) to the variance's own error, 2 / N of the bound at most
        assert ex.n > 20 and r_mean <= 1.0 and r_var <= 1.0 + 2.0 / ex.n
        ref, rmin, rmax = P.normalize(tracks, np.float64(mean), np.float64(std))
        assert (vmin, vmax) == (rmin, rmax)
        for u, r in zip(utts, ref):
            got = np.load(os.path.join(out_dir, kind, f"{u['speaker']}-{kind}-{u['basename']}.npy"))
            same_bits(got, r)
    for u in utts:
        d = np.load(os.path.join(out_dir, "duration", f"{u['speaker']}-duration-{u['basename']}.npy"))
        m = np.load(os.path.join(out_dir, "mel", f"{u['speaker']}-mel-{u['basename']}.npy"))
        assert d.dtype == np.int64 and (d == u["durations"]).all() and m.shape == (d.sum(), 80) and m.dtype == np.float32

    ds = Dataset("train.txt", pc, mc, tc, sort=True)
    assert len(ds) == 4
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])[0]
    assert len(batch) == 15 and batch[12].shape == batch[14].shape  # pitch and duration per phoneme
    model = fs2amd.FastSpeech2(pc, mc).to(DEV).eval()
    with torch.no_grad():
        out = model(*(to_device(batch, DEV)[2:]))
    torch.cuda.synchronize()
    assert out[1].shape == (4, int(batch[11]), 80) and torch.isfinite(out[1].float()).all()
