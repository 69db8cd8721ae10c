#!/usr/bin/env python3
"""Writes tests/golden/vad_a.npz: the recorded outputs of the numpy restatement tests/_vad.py
(include/fs2hip_vad.h) for the cases of _vad.fixture_cases(): per case the frame power P, the mask after
the fill, the intervals and the trim, and the waveform itself where it is short (the long rows are
rebuilt by _vad's deterministic builders). Nothing here runs on a GPU or reads anything outside tests/.

    python tests/golden/gen_golden_vad.py

The generator refuses to write unless its own conditions hold: no decision of a non-tie case lies
within a factor 2^-20 of its threshold, the tie case is a tie, and every listed edge case is there.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _vad as V  # noqa: E402

WAV_MAX = 10000  # samples of a stored waveform


def main():
    out = {}
    cases = V.fixture_cases()
    for name, (x, kw) in cases.items():
        r = V.analyse(x, **kw)
        assert V.closest_decision(r["P"], r["threshold"], r["floor"]) > 2.0 ** -20, name  # no fragile decision
        if len(x) <= WAV_MAX:
            out["wav_" + name] = x
        out["P_" + name] = r["P"]
        out["act_" + name] = r["active"].astype(np.uint8)
        out["iv_" + name] = r["intervals"]
        out["trim_" + name] = r["trim"]
    out["names"] = np.array(sorted(cases))

    # the listed edge cases
    lens = sorted(len(cases[n][0]) for n in cases if n.startswith("len_"))
    assert lens == sorted((0, 1, 255, 256, 257, 511, 512, 513, 1024, 3001, 9001))
    assert len(cases["len_5_0"][0]) == 0  # the empty row in the middle of the launch
    for c in ("silent", "constant", "first_frame", "last_frame", "impulse_0", "impulse_last", "below_floor"):
        assert "content_" + c in cases
    assert out["act_content_silent"].all() and out["act_content_constant"].all()  # ref = floor: all frames "active"
    assert out["act_content_first_frame"].tolist() == [1, 1, 1] + [0] * 13
    assert out["act_content_last_frame"].tolist() == [0] * 14 + [1, 1]
    bf = cases["content_below_floor"][0]
    assert bf.dtype == np.float32 and 0 < out["P_content_below_floor"].max() < V.floor_of(np.float32)
    for L, hop in ((2048, 512), (1200, 300), (1000, 333), (640, 640), (2, 1)):
        assert f"geo_{L}_{hop}_i16" in cases and f"geo_{L}_{hop}_f32" in cases
    f32 = cases["geo_1024_256_f32"][0].astype(np.float64) * 32768
    assert np.abs(f32 - np.round(f32)).max() > 1e-3  # not dyadic multiples of 1 / 32768
    gaps = [b[0] // 256 - a[1] // 256 for a, b in zip(out["iv_fill_1"][:-1], out["iv_fill_1"][1:])]
    assert gaps == [1, 2, 3, 7, 8], gaps
    assert [len(out[f"iv_fill_{m}"]) for m in (1, 2, 3, 8)] == [6, 5, 4, 2]  # a gap of 8 is not shorter than 8
    assert len(out["iv_nine_runs"]) == 9
    n = len(cases["margin_0"][0])
    assert out["trim_margin_1000000"].tolist() == [0, n] and (out["trim_margin_100"] - out["trim_margin_0"]).tolist() == [-100, 100]
    ch = out["act_chunks"]
    C = V.CHUNK_FRAMES
    assert len(ch) > 3 * C and ch[C - 2:C + 2].all()          # an active run across the first step boundary
    raw = V.analyse(cases["chunks"][0])["active"]
    assert not raw[2 * C - 1] and not raw[2 * C] and raw[2 * C - 2] and raw[2 * C + 1]  # a silence of 2 across the second
    assert ch[2 * C - 2:2 * C + 2].all()                       # ... filled with min_silence 3
    # the tie: exactly on the threshold in one row, above it in the other
    quiet, loud = V.tie_rows()
    rq, rl = V.analyse(quiet, threshold=V.TIE_THRESHOLD), V.analyse(loud, threshold=V.TIE_THRESHOLD)
    assert rq["P"].max() == rq["P"][4] == 400.0 and rq["P"][14] == 100.0 == V.TIE_THRESHOLD * 400.0 and rl["P"][14] == 121.0
    assert not rq["active"][14] and rl["active"][14]
    for tag, r in (("tie_quiet", rq), ("tie_loud", rl)):
        out["P_" + tag], out["act_" + tag] = r["P"], r["active"].astype(np.uint8)
        out["iv_" + tag], out["trim_" + tag] = r["intervals"], r["trim"]
    path = os.path.join(HERE, "vad_a.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print(f"wrote {path}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
