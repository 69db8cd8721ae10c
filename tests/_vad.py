"""include/fs2hip_vad.h restated in plain numpy, operation for operation: frame power in the header's
order (np.cumsum is a strictly sequential chain, one rounded add per element; numpy has no fused
multiply-add), activity, the short-silence fill, intervals, trim and cut. The oracle of the silence
tests, and the cases they share with tests/golden/gen_golden_vad.py.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L0, HOP0 = 1024, 256
CHUNK_FRAMES = 256  # FS2_VAD_CHUNK_FRAMES
TILE_FRAMES = 192   # FS2_VAD_TILE_FRAMES


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "vad_a.npz")))


def frames(n, hop):
    return 0 if n < 1 else 1 + n // hop


def threshold_of(top_db):
    return 10 ** (-top_db / 10)


def floor_of(dtype):
    """(1e-5 * full_scale) ** 2: full_scale 32768 for int16, 1.0 for float32."""
    return (1e-5 * (32768.0 if np.dtype(dtype) == np.int16 else 1.0)) ** 2


LEAF = 8


def tree(v):
    """The header's T along the last axis: neighbours added pairwise, level by level, a last element
    without a partner carried up unchanged."""
    v = np.asarray(v, dtype=np.float64)
    while v.shape[-1] > 1:
        m = v.shape[-1]
        nxt = v[..., 0:m - m % 2:2] + v[..., 1:m:2]
        v = np.concatenate([nxt, v[..., m - 1:]], axis=-1) if m % 2 else nxt
    return v[..., 0]


def frame_power(x, frame_length, hop):
    """P float64 [F] of one row (int16 or float32) in the header's order."""
    import math

    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.int16, np.float32) and 1 <= hop <= frame_length
    n, L = len(x), int(frame_length)
    F = frames(n, hop)
    if F == 0:
        return np.zeros(0)
    g = math.gcd(L, hop)
    q, h = L // g, hop // g
    nb = (F - 1) * h + q
    z = np.zeros(nb * g)  # block k = samples [k g - L // 2, (k + 1) g - L // 2), zero padded
    m = min(n, len(z) - L // 2)  # samples behind the last frame's end belong to no frame
    z[L // 2:L // 2 + m] = x[:m].astype(np.float64)
    sq = (z * z).reshape(nb, g)
    leaves = np.stack([np.cumsum(sq[:, i:i + LEAF], axis=1)[:, -1] for i in range(0, g, LEAF)], axis=1)  # sequential
    S = tree(leaves)
    idx = np.arange(F)[:, None] * h + np.arange(q)[None, :]
    return tree(S[idx]) / float(L)


def direct_power(x, frame_length, hop):
    """The same frames summed by math.fsum (correctly rounded), O(F L): what the order is measured against."""
    import math

    x = np.asarray(x).astype(np.float64)
    n, L = len(x), int(frame_length)
    out = []
    for f in range(frames(n, hop)):
        a = f * hop - L // 2
        seg = x[max(a, 0):max(min(a + L, n), 0)]
        out.append(math.fsum((seg * seg).tolist()) / L)
    return np.array(out)


def activity(P, threshold, floor):
    """The raw mask: max(P, floor) > threshold * max(max P, floor)."""
    P = np.asarray(P, dtype=np.float64)
    ref = max(float(P.max(initial=0.0)), floor)
    return np.maximum(P, floor) > np.float64(threshold) * np.float64(ref)


def runs_of(mask):
    """[(s, e)] of the maximal True runs."""
    m = np.concatenate([[False], np.asarray(mask, dtype=bool), [False]])
    d = np.flatnonzero(m[1:] != m[:-1])
    return [(int(s), int(e)) for s, e in zip(d[0::2], d[1::2])]


def fill(mask, min_silence):
    """Inactive runs shorter than min_silence strictly between two active frames become active."""
    out = np.asarray(mask, dtype=bool).copy()
    rs = runs_of(out)
    for (_, e0), (s1, _) in zip(rs[:-1], rs[1:]):
        if s1 - e0 < min_silence:
            out[e0:s1] = True
    return out


def intervals(mask, hop, n):
    """int64 [k, 2] of the (filled) mask's runs in samples."""
    return np.array([(s * hop, min(n, e * hop)) for s, e in runs_of(mask)], dtype=np.int64).reshape(-1, 2)


def trim(mask, hop, n, margin=0):
    idx = np.flatnonzero(mask)
    if len(idx) == 0:
        return 0, 0
    return max(0, int(idx[0]) * hop - margin), min(n, (int(idx[-1]) + 1) * hop + margin)


def analyse(x, *, frame_length=L0, hop=HOP0, threshold=None, top_db=60.0, floor=None, min_silence=1, margin=0):
    """Everything the kernels give for one row: dict(P, raw, active, intervals, trim, cut)."""
    x = np.asarray(x)
    thr = threshold_of(top_db) if threshold is None else threshold
    flo = floor_of(x.dtype) if floor is None else floor
    P = frame_power(x, frame_length, hop)
    raw = activity(P, thr, flo)
    act = fill(raw, min_silence)
    s, e = trim(act, hop, len(x), margin)
    return dict(P=P, raw=raw, active=act, intervals=intervals(act, hop, len(x)), trim=np.array([s, e], dtype=np.int64),
                cut=x[s:e].copy(), threshold=thr, floor=flo)


def closest_decision(P, threshold, floor):
    """min over frames of |max(P, floor) / (threshold * ref) - 1|: how far the closest decision is from a tie."""
    P = np.asarray(P, dtype=np.float64)
    if len(P) == 0:
        return np.inf
    ref = max(float(P.max()), floor)
    return float(np.abs(np.maximum(P, floor) / (threshold * ref) - 1.0).min())


def pack(arrays, dtype):
    lens = np.array([len(a) for a in arrays], dtype=np.int64)
    out = np.zeros((len(arrays), max(int(lens.max(initial=0)), 1)), dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out, lens


# ---- the shared cases -------------------------------------------------------------------------------

def _rng(seed):
    return np.random.RandomState(seed)


def burst(n, spans, amp=8000, seed=0, dtype=np.int16):
    """n samples of silence with noise of amplitude amp over the (start, end) sample spans."""
    x = np.zeros(n, dtype=np.float64)
    g = _rng(seed)
    for s, e in spans:
        x[s:e] = g.uniform(-amp, amp, e - s)
    return np.round(x).astype(np.int16) if dtype == np.int16 else (x / 32768.0 * 1.0001).astype(np.float32)


def frame_mask_row(pattern, hop=HOP0, amp=8000, seed=0):
    """An int16 row whose frames (hop-aligned blocks of noise, frame_length 4 hop) follow ``pattern``
    loosely: block k is loud where pattern[k] is true. Loud blocks are at least 4 apart or adjacent, so
    that with top_db 60 the mask is: frame f active iff any of blocks f - 2 .. f + 1 is loud."""
    pattern = np.asarray(pattern, dtype=bool)
    x = np.zeros(len(pattern) * hop, dtype=np.float64)
    g = _rng(seed)
    for k in np.flatnonzero(pattern):
        x[k * hop:(k + 1) * hop] = g.uniform(amp / 2, amp, hop) * g.choice([-1, 1], hop)
    return np.round(x).astype(np.int16)


def gaps_row():
    """Loud single blocks separated so that the silent gaps between the active frame runs are 1, 2, 3, 7
    and 8 frames (frame_length 1024, hop 256: one loud block k makes frames k - 1 .. k + 2 active)."""
    pat = np.zeros(80, dtype=bool)
    k = 3
    pat[k] = True
    for gap in (1, 2, 3, 7, 8):
        k += 4 + gap
        pat[k] = True
    return frame_mask_row(pat, seed=5)


def nine_runs_row():
    pat = np.zeros(9 * 8 + 4, dtype=bool)
    pat[2::8] = True
    return frame_mask_row(pat[:74], seed=6)


def chunk_row():
    """More than three steps of the interval kernel's walk (frame_length 1024, hop 256; a loud block k
    makes frames k - 1 .. k + 2 active): an active run across the first step boundary (frames 250 ..
    261) and, with min_silence 3, a short silence across the second (frames 504 .. 510 active, 511 and
    512 silent, 513 .. 516 active)."""
    nf = 3 * CHUNK_FRAMES + 40
    pat = np.zeros(nf, dtype=bool)
    pat[10] = True
    pat[251:260] = True
    pat[505:509] = True
    pat[514] = True
    pat[3 * CHUNK_FRAMES + 20] = True
    return frame_mask_row(pat, seed=7)


TIE_THRESHOLD = 0.25


def tie_rows():
    """(quiet, loud) int16 rows for frame_length 1024 / hop 256 and threshold 0.25. Frame f covers samples
    [256 f - 512, 256 f + 512): frame 4 lies wholly in samples of value 20, P = 400 exactly, the row's
    maximum; frame 14 lies wholly in samples of value 10, P = 100 = 0.25 * 400 exactly (``quiet``), or
    of value 11, P = 121 (``loud``)."""
    quiet = np.zeros(5120, dtype=np.int16)
    quiet[512:1536] = 20
    quiet[3072:4096] = 10
    loud = quiet.copy()
    loud[3072:4096] = 11
    return quiet, loud


LENGTHS = (1, 255, 256, 257, 511, 0, 512, 513, 1024, 3001, 9001)


def length_rows():
    """The ragged launch of the row-length case: a zero-length row in the middle."""
    g = _rng(11)
    return [np.round(g.uniform(-6000, 6000, n)).astype(np.int16) for n in LENGTHS]


def content_rows():
    n = 4000
    rows = {"silent": np.zeros(n, dtype=np.int16), "constant": np.full(n, 1234, dtype=np.int16)}
    first = np.zeros(n, dtype=np.int16)
    first[:100] = 9000
    last = np.zeros(n, dtype=np.int16)
    last[n - 40:] = 9000
    imp0 = np.zeros(n, dtype=np.int16)
    imp0[0] = 20000
    impn = np.zeros(n, dtype=np.int16)
    impn[n - 1] = 20000
    rows.update(first_frame=first, last_frame=last, impulse_0=imp0, impulse_last=impn)
    below = np.full(n, 1e-7, dtype=np.float32)  # power 1e-14 < floor 1e-10, not zero
    rows["below_floor"] = below
    return rows


def speechlike(n, seed, dtype=np.int16):
    """Silence, a burst, an inner pause, a burst, silence; with a faint noise bed 70 dB down."""
    a, b, c, d = n // 6, n // 2 - n // 12, n // 2 + n // 12, n - n // 5
    x = burst(n, [(a, b), (c, d)], amp=9000, seed=seed, dtype=np.int16).astype(np.float64)
    x += _rng(seed + 100).uniform(-2.5, 2.5, n)
    if dtype == np.int16:
        return np.round(x).astype(np.int16)
    return (x / 32768.0 * np.float32(1.00037)).astype(np.float32)  # not dyadic multiples of 1 / 32768


GEOMETRIES = ((1024, 256), (2048, 512), (1200, 300), (1000, 333), (640, 640), (2, 1))


def fixture_cases():
    """name -> (row, dict of analyse's keyword arguments): every case whose outputs the fixture records."""
    cases = {}
    for b, x in enumerate(length_rows()):
        cases[f"len_{b}_{len(x)}"] = (x, {})
    for name, x in content_rows().items():
        cases["content_" + name] = (x, {})
    for L, hop in GEOMETRIES:
        n = 7013 if hop > 1 else 301
        cases[f"geo_{L}_{hop}_i16"] = (speechlike(n, 21), dict(frame_length=L, hop=hop))
        cases[f"geo_{L}_{hop}_f32"] = (speechlike(n, 22, np.float32), dict(frame_length=L, hop=hop))
    for ms in (1, 2, 3, 8):
        cases[f"fill_{ms}"] = (gaps_row(), dict(min_silence=ms))
    for m in (0, 100, 10 ** 6):
        cases[f"margin_{m}"] = (speechlike(6000, 23), dict(margin=m))
    cases["nine_runs"] = (nine_runs_row(), {})
    cases["chunks"] = (chunk_row(), dict(min_silence=3))
    cases["top_db_40_f32"] = (speechlike(9001, 24, np.float32), dict(top_db=40.0, min_silence=2))
    return cases
