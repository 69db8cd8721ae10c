"""Silence trimming and splitting, host side (no GPU): the numpy restatement of tests/_vad.py against
the fixture tests/golden/vad_a.npz and against a correctly rounded frame power, the frame count, the
fill, interval and trim rules on hand-built masks, the tie, the size helpers and the C ABI of
include/fs2hip_vad.h."""
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest
import torch  # noqa: F401

import _vad as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_vad.h")


@pytest.fixture(scope="module")
def fx():
    return V.load_fixture()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def test_restatement_reproduces_the_fixture(fx):
    assert os.path.getsize(os.path.join(V.GOLDEN, "vad_a.npz")) < 400 * 1024
    cases = V.fixture_cases()
    assert sorted(cases) == [str(n) for n in fx["names"]]
    for name, (x, kw) in cases.items():
        if "wav_" + name in fx:
            same_bits(fx["wav_" + name], x)
        r = V.analyse(x, **kw)
        same_bits(r["P"], fx["P_" + name])
        same_bits(r["active"].astype(np.uint8), fx["act_" + name])
        same_bits(r["intervals"], fx["iv_" + name])
        same_bits(r["trim"], fx["trim_" + name])
        assert V.closest_decision(r["P"], r["threshold"], r["floor"]) > 2.0 ** -20, name


def test_power_order_is_within_4_ulp_of_the_exact_sum():
    """Float input: the header's pairwise order against math.fsum over each frame's own samples, O(F L).
    Integer input: every sum is exact, so the two agree bit for bit."""
    for L, hop in V.GEOMETRIES:
        for seed in (22, 31):
            x = V.speechlike(7013 if hop > 1 else 301, seed, np.float32)
            P, D = V.frame_power(x, L, hop), V.direct_power(x, L, hop)
            assert P.shape == D.shape == (V.frames(len(x), hop),)
            ulps = np.abs(P - D) / np.spacing(D)
            assert ulps.max() <= 4, (L, hop, ulps.max())
        xi = V.speechlike(5001 if hop > 1 else 301, 23)
        same_bits(V.frame_power(xi, L, hop), V.direct_power(xi, L, hop))


def test_int16_and_its_float_twin_give_the_same_mask():
    x = V.speechlike(9001, 41)
    twin = (x.astype(np.float64) / 32768.0).astype(np.float32)
    assert (twin.astype(np.float64) * 32768.0 == x).all()
    a, b = V.analyse(x), V.analyse(twin)
    same_bits(a["P"], b["P"] * 32768.0 ** 2)  # powers of two scale exactly
    assert np.array_equal(a["active"], b["active"]) and np.array_equal(a["intervals"], b["intervals"])


def test_frame_count_rule():
    for hop in (1, 2, 256, 333):
        for n, want in ((0, 0), (1, 1 + 1 // hop), (hop - 1, 1 if hop > 1 else 0), (hop, 2), (hop + 1, 2 + (hop == 1)),
                        (2 * hop, 3)):
            assert V.frames(n, hop) == want, (n, hop)
            x = np.ones(n, dtype=np.int16)
            assert len(V.frame_power(x, max(hop, 2), hop)) == want


def test_frames_are_centred_and_zero_padded():
    x = np.arange(1, 11, dtype=np.int16)  # frame_length 4, hop 2: frame f covers [2 f - 2, 2 f + 2)
    P = V.frame_power(x, 4, 2)
    want = [(1 + 4) / 4, (1 + 4 + 9 + 16) / 4, (9 + 16 + 25 + 36) / 4, (25 + 36 + 49 + 64) / 4, (49 + 64 + 81 + 100) / 4,
            (81 + 100) / 4]
    assert P.tolist() == want
    P3 = V.frame_power(x, 5, 3)  # hop does not divide frame_length: frame f covers [3 f - 2, 3 f + 3)
    assert P3.tolist() == [(1 + 4 + 9) / 5, (4 + 9 + 16 + 25 + 36) / 5, (25 + 36 + 49 + 64 + 81) / 5, (64 + 81 + 100) / 5]


def test_trim_and_split_on_hand_built_masks():
    m = np.array([0, 0, 1, 1, 0, 1, 0, 0], dtype=bool)
    assert V.intervals(m, 10, 75).tolist() == [[20, 40], [50, 60]]
    assert V.trim(m, 10, 75) == (20, 60) and V.trim(m, 10, 75, margin=7) == (13, 67)
    assert V.trim(m, 10, 75, margin=30) == (0, 75)
    last = np.array([0, 1, 1], dtype=bool)
    assert V.intervals(last, 10, 25).tolist() == [[10, 25]] and V.trim(last, 10, 25) == (10, 25)  # clamped to n
    none = np.zeros(5, dtype=bool)
    assert V.intervals(none, 10, 45).shape == (0, 2) and V.trim(none, 10, 45, margin=100) == (0, 0)
    assert V.intervals(np.ones(3, dtype=bool), 10, 25).tolist() == [[0, 25]]


def test_fill_rule():
    def mask(s):
        return np.array([c == "x" for c in s])

    def text(m):
        return "".join("x" if v else "." for v in m)

    row = "..x.x..x...x.."  # gaps of 1, 2 and 3 between active frames, inactive runs of 2 at both ends
    assert text(V.fill(mask(row), 1)) == row
    assert text(V.fill(mask(row), 2)) == "..xxx..x...x.."
    assert text(V.fill(mask(row), 3)) == "..xxxxxx...x.."
    assert text(V.fill(mask(row), 4)) == "..xxxxxxxxxx.."
    assert text(V.fill(mask(row), 100)) == "..xxxxxxxxxx.."  # the ends are never filled
    assert text(V.fill(mask("....."), 9)) == "....." and text(V.fill(mask("x...."), 9)) == "x...."


def test_tie_is_inactive_and_one_count_louder_is_active(fx):
    quiet, loud = V.tie_rows()
    rq, rl = V.analyse(quiet, threshold=V.TIE_THRESHOLD), V.analyse(loud, threshold=V.TIE_THRESHOLD)
    assert rq["P"][4] == 400.0 == rq["P"].max() and rq["P"][14] == 100.0 and rl["P"][14] == 121.0
    assert V.TIE_THRESHOLD * 400.0 == 100.0
    assert not rq["active"][14] and rl["active"][14] and rq["active"][4] and rl["active"][4]
    assert int((loud != quiet).sum()) == 1024 and int((loud - quiet).max()) == 1
    same_bits(rq["active"].astype(np.uint8), fx["act_tie_quiet"])
    same_bits(rl["active"].astype(np.uint8), fx["act_tie_loud"])


def test_size_mirror_agrees_with_the_standalone_check():
    """tools/vad_sizes_check.py: the stand-alone host program over csrc/vad_sizes.h compares the header
    with a 128-bit restatement up to INT32_MAX and prints what the Python mirror has to give. The tool's
    own run builds it with ASan and UBSan (DESIGN 9.8 records that run); here the same program is built
    plainly, so that the comparison does not depend on a sanitizer runtime."""
    spec = importlib.util.spec_from_file_location("vad_sizes_check", os.path.join(REPO, "tools", "vad_sizes_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cxx = shutil.which("g++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler build() uses otherwise
    assert mod.check(cxx, sanitize=False) > 10000


def test_vad_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_VAD) == ["fs2_vad_cut", "fs2_vad_frames", "fs2_vad_intervals",
                                                       "fs2_vad_lds_bytes", "fs2_vad_power",
                                                       "fs2_vad_workspace_bytes"], declared
    assert "fs2hip_vad.h" in _lib.EXTRA_HEADERS and _lib.HEADER_VAD == HEADER
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    ctype = {"int": _lib._i, "int64_t": _lib._i64, "double": _lib._d, "fs2_stream_t": _lib._p}
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_VAD[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m and ctype[m.group(1)] is res, name
        params = [p.strip() for p in m.group(2).split(",")]
        want = [_lib._p if "*" in p else ctype[p.split()[0]] for p in params]
        assert want == list(args), (name, params)
    raw = open(HEADER).read()
    for name, val in (("FS2_VAD_SUMS_BYTES", _lib.VAD_SUMS_BYTES), ("FS2_VAD_AREA_BYTES", _lib.VAD_AREA_BYTES),
                      ("FS2_VAD_TILE_FRAMES", _lib.VAD_TILE_FRAMES), ("FS2_VAD_CHUNK_FRAMES", _lib.VAD_CHUNK_FRAMES),
                      ("FS2_VAD_B_MAX", _lib.VAD_B_MAX)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", raw).group(1)) == val, name
    assert V.CHUNK_FRAMES == _lib.VAD_CHUNK_FRAMES and V.TILE_FRAMES == _lib.VAD_TILE_FRAMES


def test_sizes_are_the_headers_formulas():
    from fs2amd import _lib

    lib = _lib.load()
    for n, hop in ((0, 256), (1, 256), (255, 256), (256, 256), (257, 256), (512, 256), (220500, 256), (5, 1)):
        assert lib.fs2_vad_frames(n, hop) == V.frames(n, hop) == _lib.vad_frames(n, hop)
    assert lib.fs2_vad_frames(10, 0) == -1
    for L, hop in V.GEOMETRIES + ((4096, 1), (4097, 1), (8191, 8191), (8192, 8192), (1024, 2048), (0, 0)):
        assert lib.fs2_vad_lds_bytes(L, hop) == _lib.vad_lds_bytes(L, hop)
        for B, F in ((1, 1), (7, 36), (64, 862), (0, 5), (5, 0)):
            assert lib.fs2_vad_workspace_bytes(B, F, L, hop) == _lib.vad_workspace_bytes(B, F, L, hop)
    assert _lib.vad_workspace_bytes(64, 862, 1024, 256) == 8 * 64 * 5 and _lib.vad_tile_frames(1000, 333) == 10
    assert _lib.vad_status(1, 100, 4096, 1) == _lib.FS2_OK and _lib.vad_status(1, 100, 4097, 1) == _lib.FS2_EUNSUPPORTED
    assert _lib.vad_status(1, 100, 8191, 8191) == _lib.FS2_OK
    assert _lib.vad_status(1, 100, 8192, 8192) == _lib.FS2_EUNSUPPORTED


def test_entries_reject_bad_arguments_without_a_gpu():
    """The argument checks come before any launch, so they answer on a machine without a device."""
    from fs2amd import _lib

    lib = _lib.load()
    p = 4096  # a non-null pointer that is never followed: every call below is refused first
    E, U = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED

    def power(wav=p, dtype=_lib.FS2_I16, stride=1000, B=2, n_max=1000, L=1024, hop=256, P=p, Pmax=p, ws=p, ws_bytes=1 << 20):
        return lib.fs2_vad_power(wav, dtype, stride, None, B, n_max, L, hop, P, Pmax, ws, ws_bytes, None)

    for kw in (dict(wav=None), dict(P=None), dict(Pmax=None), dict(ws=None), dict(B=0), dict(n_max=0), dict(L=0),
               dict(hop=0), dict(hop=-1), dict(L=256, hop=257), dict(stride=999), dict(ws_bytes=8)):
        assert power(**kw) == E, kw
    for kw in (dict(dtype=_lib.FS2_F64), dict(dtype=_lib.FS2_BF16), dict(B=65536), dict(L=4097, hop=1),
               dict(L=8192, hop=8192), dict(n_max=2 ** 31 - 1, stride=2 ** 31 - 1, L=2, hop=1),
               dict(B=65535, n_max=2 ** 24, stride=2 ** 24, hop=256)):
        assert power(**kw) == U, kw

    def intervals(P=p, Pmax=p, B=2, n_max=1000, hop=256, thr=0.01, floor=0.1, ms=1, margin=0, cap=4, chunk=0, act=p,
                  count=p, iv=p, trim=p):
        return lib.fs2_vad_intervals(P, Pmax, None, B, n_max, hop, thr, floor, ms, margin, cap, chunk, act, count, iv,
                                     trim, None)

    for kw in (dict(P=None), dict(Pmax=None), dict(act=None), dict(count=None), dict(iv=None), dict(trim=None), dict(B=0),
               dict(n_max=0), dict(hop=0), dict(ms=0), dict(margin=-1), dict(cap=-1), dict(chunk=100), dict(chunk=512),
               dict(thr=-0.5), dict(thr=float("nan")), dict(floor=-1.0), dict(floor=float("nan"))):
        assert intervals(**kw) == E, kw
    for kw in (dict(B=65536), dict(n_max=2 ** 31 - 1, hop=1), dict(B=65535, n_max=2 ** 24), dict(B=65535, cap=2 ** 20)):
        assert intervals(**kw) == U, kw

    def cut(wav=p, dtype=_lib.FS2_I16, stride=1000, trim=p, B=2, n_max=1000, M=10, out=p):
        return lib.fs2_vad_cut(wav, dtype, stride, trim, B, n_max, M, out, None, None)

    for kw in (dict(wav=None), dict(trim=None), dict(out=None), dict(B=0), dict(n_max=0), dict(M=0), dict(stride=999)):
        assert cut(**kw) == E, kw
    for kw in (dict(dtype=_lib.FS2_F64), dict(B=65536)):
        assert cut(**kw) == U, kw


def test_api_is_exported_and_keeps_its_defaults():
    import inspect

    import fs2amd
    from fs2amd import ops, preprocess

    for name in ("trim_silence", "split_silence"):
        assert name in fs2amd.__all__ and getattr(fs2amd, name) is getattr(preprocess, name)
        sig = inspect.signature(getattr(fs2amd, name)).parameters
        assert (sig["top_db"].default, sig["frame_length"].default, sig["hop_length"].default,
                sig["min_silence"].default) == (60.0, 2048, 512, 1)  # librosa's
    assert inspect.signature(fs2amd.trim_silence).parameters["margin"].default == 0
    sig = inspect.signature(fs2amd.prepare_wavs).parameters
    assert (sig["trim_db"].default, sig["trim_frame_length"].default, sig["trim_hop_length"].default,
            sig["trim_margin"].default) == (None, 2048, 512, 0)
    sig = inspect.signature(fs2amd.build_corpus).parameters
    assert sig["trim_db"].default is None and sig["trim_margin"].default == 0
    for name in ("frame_power", "activity_intervals", "cut_rows"):
        assert callable(getattr(ops, name))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_power(torch.zeros(1, 100, dtype=torch.int16), frame_length=64, hop_length=16)
    thr, floor = preprocess._vad_params(60.0, np.int16)
    assert thr == V.threshold_of(60.0) == 10 ** -6.0 and floor == V.floor_of(np.int16) == (1e-5 * 32768.0) ** 2
    assert preprocess._vad_params(40.0, np.float32) == (V.threshold_of(40.0), V.floor_of(np.float32))
