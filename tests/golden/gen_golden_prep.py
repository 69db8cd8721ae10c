#!/usr/bin/env python3
"""Generate tests/golden/prep_a.npz from the REFERENCE's preprocessing arithmetic on the CPU.

Runs only where the reference tree is mounted (FS2_REFERENCE, default /root/reference) and scipy
and scikit-learn are installed; only the .npz travels. ``librosa``, ``pyworld``, ``tgt`` and ``tqdm``
are not installed: stand-in modules go into ``sys.modules`` so that preprocessor/preprocessor.py
imports (none of their functions is called). A ``Preprocessor`` is made without its ``__init__``
(which reads corpus files) and its own ``remove_outlier`` and ``normalize`` (on a temporary
directory) are called; the interpolation is ``scipy.interpolate.interp1d`` as :275-281 calls it, the
phoneme means are the loop of :283-291 (it sits inside ``process_utterance`` behind pyworld and
cannot be called alone), the statistics are ``sklearn.preprocessing.StandardScaler.partial_fit`` in
the order of ``build_from_path`` (:152-155).

The restatement in tests/_prep.py must equal all of these before anything is written: masks,
quartiles (against ``np.percentile`` in each dtype), interpolated contours, normalised values,
minimum and maximum bit for bit.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_prep.py
"""
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FS2_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _prep as P  # noqa: E402
from _npz_parts import save_npz_parts  # noqa: E402
from gen_golden_audio import install_librosa_stand_ins  # noqa: E402

TRACK_LENS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 2049]


def import_reference_preprocessor():
    install_librosa_stand_ins()
    sys.modules["librosa"].load = None
    for name in ("pyworld", "tgt", "tqdm"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].tqdm = lambda x, **k: x
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import preprocessor.preprocessor as ref
    assert ref.__file__.startswith(REF)
    return ref


def contour(T, runs, rng):
    """A smooth contour (two slow sines around 180 Hz) that is non-zero on runs [(a, b), ...]."""
    t = np.arange(T)
    y = 180.0 + 40.0 * np.sin(t / 17.0 + rng.uniform(0, 6)) + 9.0 * np.sin(t / 3.1 + rng.uniform(0, 6))
    out = np.zeros(T)
    for a, b in runs:
        out[a:b] = y[a:b]
    return out


def durations(total, L, rng, zero_at):
    """L non-negative integers of sum total, zero at the indices zero_at (none first), with
    sum(d[:i]) >= i for every i."""
    while True:
        cuts = np.sort(rng.integers(0, total + 1, size=L - 1))
        d = np.diff(np.concatenate([[0], cuts, [total]]))
        for z in zero_at:
            d[z - 1] += d[z]
            d[z] = 0
        if d[0] >= 2 and all(d[:i].sum() >= i for i in range(L)):
            return d.astype(np.int64)


def pitch_cases(rng):
    cases = [  # (name, contour, durations)
        ("lead_trail_T300_crop", contour(300, [(23, 61), (64, 130), (131, 132), (190, 266)], rng),
         durations(290, 31, rng, (4, 17))),
        ("single_between_gaps_T129", contour(129, [(0, 40), (70, 71), (100, 129)], rng), durations(129, 14, rng, (3,))),
        ("fully_voiced_T64", contour(64, [(0, 64)], rng), durations(64, 9, rng, (2, 5))),
        ("two_voiced_T65", contour(65, [(5, 6), (50, 51)], rng), durations(65, 8, rng, (6,))),
        ("one_voiced_T63_dropped", contour(63, [(31, 32)], rng), durations(63, 7, rng, ())),
        ("none_voiced_T2_dropped", np.zeros(2), np.array([2], dtype=np.int64)),
        ("one_frame_T1_dropped", np.array([123.25]), np.array([1], dtype=np.int64)),
        ("two_frames_T2", np.array([101.5, 97.125]), np.array([1, 1], dtype=np.int64)),
        # three passes of 256 frames: gaps that cross a wave and a pass boundary, voiced at 255 | 256
        ("three_passes_T700", contour(700, [(3, 50), (120, 200), (255, 257), (330, 331), (333, 500), (640, 690)], rng),
         durations(700, 64, rng, (1, 30, 63))),
    ]
    for name, f0, d in cases:
        assert all(d[:i].sum() >= i for i in range(len(d))) and d.sum() <= len(f0), name
    assert any((d[1:] == 0).any() for _, _, d in cases)
    return cases


def value_tracks(rng):
    """(float64 pitch-like track, float32 energy-like track) per utterance, lengths TRACK_LENS, plus
    the special ones."""
    t64, t32 = [], []
    for n in TRACK_LENS:
        p = 200.0 + 40.0 * rng.standard_normal(n)
        e = (30.0 + 20.0 * rng.standard_normal(n)).astype(np.float32)
        if n >= 63:  # heavy tails: a few far outliers on both sides
            k = max(n // 40, 2)
            p[rng.integers(0, n, k)] *= rng.choice([0.2, 2.5], k)
            e[rng.integers(0, n, k)] *= np.float32(4.0)
        t64.append(p)
        t32.append(e)
    # repeated values
    t64.append(np.round(200.0 + 40.0 * rng.standard_normal(200), -1))
    t32.append(np.round(30.0 + 20.0 * rng.standard_normal(200)).astype(np.float32))
    # an element exactly on the upper fence: p25 = 2, p75 = 6, upper = 6 + 1.5 * 4 = 12
    fence = np.array([5, 1, 12, 0, 7, 3, 2, 6, 4], dtype=np.float32)
    t64.append(fence.astype(np.float64) * 10.0)
    t32.append(fence)
    return t64, t32


def main():
    from scipy.interpolate import interp1d
    from sklearn.preprocessing import StandardScaler

    ref = import_reference_preprocessor()
    pre = ref.Preprocessor.__new__(ref.Preprocessor)
    rng = np.random.default_rng(20261)
    out = {}

    # ---- pitch targets
    cases = pitch_cases(rng)
    f0s, durs, filled, ph, voiced = [], [], [], [], []
    for name, f0, d in cases:
        pitch = f0[:sum(d)]  # :263
        nz = int(np.sum(pitch != 0))
        r_ph, r_filled, r_voiced = P.pitch_target(f0, d)
        assert r_voiced == nz, name
        if nz <= 1:  # :264-265
            assert r_ph is None and "dropped" in name, name
            ref_filled, ref_ph = np.zeros(0), np.zeros(0)
        else:
            ids = np.where(pitch != 0)[0]
            fn = interp1d(ids, pitch[ids], fill_value=(pitch[ids[0]], pitch[ids[-1]]), bounds_error=False)
            ref_filled = fn(np.arange(0, len(pitch)))
            work = ref_filled.copy()
            pos = 0
            for i, dd in enumerate(d):  # :284-291
                if dd > 0:
                    work[i] = np.mean(work[pos:pos + dd])
                else:
                    work[i] = 0
                pos += dd
            ref_ph = work[:len(d)]
            assert ref_filled.dtype == np.float64 and np.array_equal(ref_filled.view(np.uint64), r_filled.view(np.uint64)), name
            assert np.array_equal(ref_ph, r_ph), name
            # the in-place loop is the plain mean here
            plain = [ref_filled[d[:i].sum():d[:i + 1].sum()].mean() if d[i] > 0 else 0.0 for i in range(len(d))]
            assert np.array_equal(ref_ph, np.array(plain)), name
        f0s.append(f0)
        durs.append(d)
        filled.append(ref_filled)
        ph.append(ref_ph)
        voiced.append(nz)
    out.update(pitch_names=np.array([c[0] for c in cases]), f0=np.concatenate(f0s),
               f0_lens=np.array([len(f) for f in f0s], dtype=np.int64), dur=np.concatenate(durs),
               dur_lens=np.array([len(d) for d in durs], dtype=np.int64), ref_filled=np.concatenate(filled),
               ref_filled_lens=np.array([len(f) for f in filled], dtype=np.int64), ref_ph=np.concatenate(ph),
               ref_ph_lens=np.array([len(p) for p in ph], dtype=np.int64), ref_voiced=np.array(voiced, dtype=np.int32))

    # ---- outlier fence, per dtype
    t64, t32 = value_tracks(rng)
    for tag, tracks in (("64", t64), ("32", t32)):
        masks, quart = [], []
        for v in tracks:
            mask, p25, p75 = P.outlier_fence(v)
            if len(v):
                kept = pre.remove_outlier(v)
                assert kept.dtype == v.dtype and np.array_equal(kept, v[mask]), (tag, len(v))
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    n25, n75 = np.percentile(v, 25), np.percentile(v, 75)
                assert n25.dtype == v.dtype and (n25, n75) == (p25, p75), (tag, len(v), n25, p25, n75, p75)
            masks.append(mask)
            quart.append([p25, p75])
        out.update({f"tracks{tag}": np.concatenate(tracks), f"mask{tag}": np.concatenate(masks),
                    f"quart{tag}": np.array(quart, dtype=tracks[0].dtype)})
    out["track_lens"] = np.array([len(v) for v in t64], dtype=np.int64)
    fence = t32[-1]
    m, p25, p75 = P.outlier_fence(fence)
    assert (p25, p75) == (2.0, 6.0) and not m[fence == 12.0].any() and m.sum() == len(fence) - 1
    assert not P.outlier_fence(t32[1])[0].any() and len(t32[1]) == 1  # n = 1: no inlier

    # ---- the scalers, in build_from_path's order (:152-155): pitch (float64) and energy (float32) per utterance
    for tag, tracks in (("64", t64), ("32", t32)):
        sc = StandardScaler()
        means, vars_, seen = [], [], []
        for v in tracks:
            kept = pre.remove_outlier(v) if len(v) else v
            if len(kept) > 0:
                sc.partial_fit(kept.reshape((-1, 1)))
            fitted = hasattr(sc, "mean_")
            means.append(sc.mean_[0] if fitted else np.nan)
            vars_.append(sc.var_[0] if fitted else np.nan)
            seen.append(int(sc.n_samples_seen_) if fitted else 0)
        out.update({f"scaler{tag}_mean": np.array(means), f"scaler{tag}_var": np.array(vars_),
                    f"scaler{tag}_n": np.array(seen, dtype=np.int64), f"scaler{tag}_scale": np.array(sc.scale_[0])})
        samples = np.concatenate([v[P.outlier_fence(v)[0]] for v in tracks])
        assert len(samples) == seen[-1]
        print(f"scaler{tag}: N = {seen[-1]}, reference ratios (mean, var) = {P.scaler_ratios(means[-1], vars_[-1], samples)}")

    # ---- normalisation through the reference's own method on a temporary directory
    def ref_normalize(tracks, mean, std):
        with tempfile.TemporaryDirectory() as tmp:
            for i, v in enumerate(tracks):
                np.save(os.path.join(tmp, f"{i:03d}.npy"), v)
            vmin, vmax = pre.normalize(tmp, mean, std)
            return [np.load(os.path.join(tmp, f"{i:03d}.npy")) for i in range(len(tracks))], vmin, vmax

    n64, n32 = [v for v in t64 if len(v)], [v for v in t32 if len(v)]
    out["norm_ids"] = np.array([i for i, v in enumerate(t64) if len(v)], dtype=np.int64)
    for tag, tracks, mean, std in (("64", n64, out["scaler64_mean"][-1], out["scaler64_scale"]),
                                   ("32", n32, out["scaler32_mean"][-1], out["scaler32_scale"]),
                                   ("32_off", n32, 0, 1)):
        vals, vmin, vmax = ref_normalize(tracks, mean, std)
        r_vals, r_min, r_max = P.normalize(tracks, mean, std)
        want = np.float32 if tag == "32_off" else np.float64
        for a, b in zip(vals, r_vals):
            assert a.dtype == b.dtype == want and np.array_equal(a, b), tag
        assert (vmin, vmax) == (r_min, r_max), tag
        out.update({f"norm{tag}": np.concatenate(vals), f"norm{tag}_minmax": np.array([vmin, vmax], dtype=np.float64)})

    n = save_npz_parts(os.path.join(HERE, "prep_a.npz"), **out)
    print("wrote prep_a.npz in", n, "part(s),", os.path.getsize(os.path.join(HERE, "prep_a.npz")), "bytes")


if __name__ == "__main__":
    main()
