"""The phase vocoder, host side (no GPU): the numpy restatement of tests/_pvoc.py against the fixture
tests/golden/pvoc_a.npz, against the angle form of librosa's rule and against the input at rate 1, on
hand-built spectra, the frame count, the duration rule, the size checks and the C ABI of
include/fs2hip_pvoc.h."""
import importlib.util
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch  # noqa: F401

import _pvoc as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_pvoc.h")


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
    assert os.path.getsize(os.path.join(V.GOLDEN, "pvoc_a.npz")) < 400 * 1024
    cases = V.fixture_cases()
    assert sorted(cases) == [str(n) for n in fx["names"]]
    assert set(fx) == {"names"} | {p + n for n in cases for p in ("out_", "J_")}  # outputs, nothing else
    for name, (spec, T, rate) in cases.items():
        got = V.pvoc(spec, T, rate)
        assert got.shape == (spec.shape[0], int(fx["J_" + name])) and got.dtype == np.float32
        same_bits(got, fx["out_" + name])
    counts = {int(fx["J_" + n]) for n in cases if n.startswith("k_")}
    assert {1, 63, 64, 65, 128, 129, 520} <= counts  # the carry crosses one, two and eight blocks


@pytest.mark.parametrize("T,rate", ((88, 1.25), (300, 1.25), (860, 0.8), (5170, 1.25)))
def test_against_the_angle_form(T, rate):
    """|rotor form - angle form| <= mag_j * 4 * J * 2^-52 * max |phase_acc|, the accumulator of the angle
    form itself: each of its J steps rounds at that magnitude, and then it is the phase error of an output
    of modulus mag_j. 71 to 4,136 output frames."""
    NB = 33
    spec = V.random_spec(NB, T, 300 + T)
    mag, Px, Py = V.pvoc64(spec, T, rate)
    ref, biggest = V.pvoc_angle(spec, T, rate)
    J = V.frames(T, rate)
    assert mag.shape == ref.shape == (NB, J) and J in (71, 240, 1075, 4136)
    diff = np.abs(mag * Px + 1j * (mag * Py) - ref)
    bound = mag * (4 * J * 2.0 ** -52 * biggest)
    ratio = (diff / np.maximum(bound, np.finfo(np.float64).tiny)).max()
    print(f"T {T} rate {rate}: J {J}, max |phase_acc| {biggest:.4g}, largest diff / bound {ratio:.4g}")
    assert biggest > J and (diff <= bound).all()
    assert np.abs(np.hypot(Px, Py) - 1.0).max() < 1e-12  # the drift of |P|, not renormalised


def test_rate_one_returns_the_input():
    NB, T = 9, 333
    spec = V.random_spec(NB, T, 41)
    out = V.pvoc(spec, T, 1.0)
    assert out.shape == spec.shape
    D = np.hypot(spec[:NB].astype(np.float64), spec[NB:].astype(np.float64))
    err = np.hypot(out[:NB].astype(np.float64) - spec[:NB], out[NB:].astype(np.float64) - spec[NB:])
    assert (err <= 2.0 ** -23 * D).all()


def test_zero_frames_and_zero_rows():
    NB, T = 5, 40
    spec = V.zero_frames_spec(NB, T)
    for rate in (0.8, 1.0, 1.25):
        mag, Px, Py = V.pvoc64(spec, T, rate)
        out = V.pvoc(spec, T, rate)
        assert np.isfinite(out).all() and np.abs(np.hypot(Px, Py) - 1.0).max() < 1e-13
        assert not out[3].any() and not out[NB + 3].any() and (Px[3] == 1.0).all() and (Py[3] == 0.0).all()
        p = np.arange(V.frames(T, rate)) * rate
        i = np.floor(p).astype(int)
        zeros = (0, 1, 2, 17, 18, 19, 20, 38, 39, 40)  # the zero frames and the pad
        dead = np.isin(i, zeros) & np.isin(i + 1, zeros)  # between two zero frames: magnitude 0
        alive = ~np.isin(i, zeros)                        # 1 - alpha > 0 times a magnitude above 0
        assert dead.any() and not out[:, dead].any() and (np.abs(out[:, alive][[0, 1, 2, 4]]) > 0).all()
    # rate 1: a zero frame has unit (1, 0); the frames behind it come back with their own phase
    one = V.pvoc(spec, T, 1.0)
    live = np.abs(spec).max(axis=0) > 0
    D = np.hypot(spec[:NB].astype(np.float64), spec[NB:].astype(np.float64))
    err = np.hypot(one[:NB].astype(np.float64) - spec[:NB], one[NB:].astype(np.float64) - spec[NB:])
    assert live[3:17].all() and live[21:38].all() and (err <= 2.0 ** -23 * D).all()
    zero = np.zeros((2 * NB, 30), dtype=np.float32)
    for rate in (0.5, 1.0, 3.0):
        out = V.pvoc(zero, 30, rate)
        assert out.shape == (2 * NB, V.frames(30, rate)) and (bits(out) == 0).all()  # +0.0, not -0.0


def test_tiny_rows():
    NB = 4
    spec = V.random_spec(NB, 2, 5)
    assert V.pvoc(spec, 0, 1.0).shape == (2 * NB, 0) and V.pvoc(spec[:, :0], 0, 0.5).shape == (2 * NB, 0)
    # T = 1: frame 0 fades into the pad; the phase is e[0] throughout (every rotor is conj(e[0]) * (1, 0)
    # only from j = 1 on, and only one more factor is ever used at rate 0.25: j = 0 .. 3 all have i = 0)
    out = V.pvoc(spec, 1, 0.25)
    re, im = spec[:NB, 0].astype(np.float64), spec[NB:, 0].astype(np.float64)
    m = np.sqrt(re * re + im * im)
    ex, ey = re / m, im / m
    assert out.shape == (2 * NB, 4)
    same_bits(out[:NB, 0], (1.0 * m * ex).astype(np.float32))
    same_bits(out[NB:, 0], (m * ey).astype(np.float32))
    rx, ry = 1.0 * ex + 0.0 * ey, 0.0 * ex - 1.0 * ey       # e[1] * conj(e[0]) with e[1] = (1, 0)
    p1 = (ex * rx - ey * ry, ex * ry + ey * rx)             # P_1 = e[0] (*) rotor_0: about (1, 0)
    same_bits(out[:NB, 1], ((0.75 * m + 0.25 * 0.0) * p1[0]).astype(np.float32))
    same_bits(out[NB:, 1], ((0.75 * m + 0.25 * 0.0) * p1[1]).astype(np.float32))
    assert V.pvoc(spec, 1, 1.0).shape == (2 * NB, 1) and V.pvoc(spec, 1, 7.0).shape == (2 * NB, 1)
    # T = 2 at rate 1 is the input
    two = V.pvoc(spec, 2, 1.0)
    assert two.shape == (2 * NB, 2) and np.abs(two - spec).max() <= 2.0 ** -23 * np.abs(spec).max()
    same_bits(two[:, 0], V.pvoc(spec, 1, 1.0)[:, 0])
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert V.pvoc(spec, 2, bad).shape == (2 * NB, 0)


def test_scan_order_is_the_headers():
    """The block scan against the definition spelt out one element at a time."""
    r = np.random.default_rng(3)
    J = 150
    ang = r.uniform(0, 6, (2, J))
    sx, sy = np.cos(ang), np.sin(ang)
    Px, Py = V.scan(sx, sy)

    def mul(a, b):
        return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])

    for row in range(2):
        want = []
        for c0 in range(0, J, V.BLOCK):
            x = [(sx[row, k], sy[row, k]) for k in range(c0, min(c0 + V.BLOCK, J))]
            d = 1
            while d < V.BLOCK:
                x = [x[k] if k < d else mul(x[k - d], x[k]) for k in range(len(x))]
                d *= 2
            if c0:
                x = [mul(want[c0 - 1], v) for v in x]
            want += x
        same_bits(Px[row], np.array([v[0] for v in want]))
        same_bits(Py[row], np.array([v[1] for v in want]))
    a, b = (sx[0], sy[0]), (sx[1], sy[1])
    same_bits(np.array(V.cmul(a, b)), np.array(V.cmul(b, a)))  # commutative bit for bit


def test_frame_count():
    from fs2amd import _lib

    lib = _lib.load()
    r = np.random.default_rng(11)
    pairs = [(int(T), float(x)) for T, x in zip(r.integers(0, 3000, 400), r.uniform(0.2, 4.0, 400))]
    pairs += [(T, x) for T in (0, 1, 2, 63, 64, 65, 130, 860) for x in V.KERNEL_RATES + (0.8, 1.25, 1.0 / 3.0, 0.1)]
    pairs += [(T, T / m) for T in (7, 64, 100, 513) for m in range(1, 3 * T)]  # quotients on or beside an integer
    for T, x in pairs:
        want = V.frames_by_definition(T, x)
        assert V.frames(T, x) == want == _lib.pvoc_frames(T, x) == lib.fs2_pvoc_frames(T, x), (T, x)
    for x in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):
        assert V.frames(100, x) == _lib.pvoc_frames(100, x) == lib.fs2_pvoc_frames(100, x) == 0
    for T, x, want in ((5, 1e-320, V.J_CAP), (5, 1e300, 1), (1 << 40, 1.0, V.J_CAP), (1, 1e-9, 10 ** 9), (-3, 1.0, 0),
                       (2 ** 31 - 1, 1.0, V.J_CAP), (2 ** 31 - 2, 1.0, 2 ** 31 - 2), (3, 1.7976931348623157e308, 1)):
        assert V.frames(T, x) == _lib.pvoc_frames(T, x) == lib.fs2_pvoc_frames(T, x) == want, (T, x)
    assert _lib.PVOC_J_CAP == V.J_CAP and _lib.PVOC_BLOCK == V.BLOCK
    same = sum(V.frames(T, x) == len(np.arange(0, T, x)) for T, x in pairs[:400])
    assert same >= 396  # numpy's own count, but for rounding edges


def test_duration_rescale_rule():
    from fs2amd.augment import rescale_durations

    d = np.array([3, 0, 5, 2, 7], dtype=np.int64)  # boundaries 3 3 8 10 17
    got = rescale_durations(d, 0.8, 256 * 21 + 5, 256)  # T' = 22; 3.75+.5 -> 4, 4, 10.5 -> 10, 13, 21.75 -> 21
    assert got.tolist() == [4, 0, 6, 3, 8] and got.dtype == np.int64
    assert rescale_durations(d, 0.8, 256 * 19, 256).tolist() == [4, 0, 6, 3, 7]  # T' = 20 caps the last boundary
    assert rescale_durations(d, 2.0, 256 * 8, 256).tolist() == [2, 0, 2, 1, 4]  # 1.5+.5 -> 2, 2, 4, 5, 9 (8.5+.5)
    assert rescale_durations(d, 1.0, 256 * 16, 256).tolist() == d.tolist()
    assert rescale_durations(d, 0.5, 100, 256).tolist() == [1, 0, 0, 0, 0]  # T' = 1
    assert rescale_durations([], 0.9, 1000, 256).tolist() == []
    r = np.random.default_rng(2)
    for _ in range(50):
        d = r.integers(0, 9, r.integers(1, 30))
        rate = float(r.uniform(0.5, 2.0))
        n_new = int(round(256 * int(d.sum()) / rate))
        got = rescale_durations(d, rate, n_new, 256)
        same_bits(got, V.rescale_durations(d, rate, n_new, 256))
        assert (got >= 0).all() and got.sum() <= 1 + n_new // 256 and len(got) == len(d)
        assert abs(int(got.sum()) - d.sum() / rate) <= 1.0


def test_pitch_fraction():
    from fs2amd.augment import PITCH_FRACTION_LIMIT, pitch_fraction

    assert pitch_fraction(12) == (2, 1) and pitch_fraction(-12) == (1, 2) and pitch_fraction(0) == (1, 1)
    assert pitch_fraction(24) == (4, 1) and pitch_fraction(7.0201) == (3, 2)  # nothing else is within 1 / 340
    for s in (-7, -2, -1, 0.5, 1, 2, 3, 5, 7):
        p, q = pitch_fraction(s)
        f = 2.0 ** (s / 12.0)
        assert (p, q) == V.closest_fraction(f) and math.gcd(p, q) == 1 and max(p, q) <= PITCH_FRACTION_LIMIT == 256
        assert abs(p / q - f) <= f / (2 * 128)  # some denominator in (128, 256] is this close
        assert all(abs(a / b - f) >= abs(p / q - f) for b in range(1, 257) for a in (int(f * b), int(f * b) + 1)
                   if 1 <= a <= 256)


def test_size_mirror_agrees_with_the_standalone_check():
    """tools/pvoc_sizes_check.py: the stand-alone host program over csrc/pvoc_sizes.h compares the header
    with the definition and prints what the Python mirror has to give. The tool's own run builds it with
    ASan and UBSan (DESIGN 9.9 records that run); here the same program is built plainly, so that the
    comparison does not depend on a sanitizer runtime."""
    spec = importlib.util.spec_from_file_location("pvoc_sizes_check", os.path.join(REPO, "tools", "pvoc_sizes_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cxx = shutil.which("g++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler build() uses otherwise
    assert mod.check(cxx, sanitize=False) > 10000


def test_pvoc_header_symbols_exported_and_bound():
    import ctypes

    import __graft_entry__ as g
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_PVOC) == ["fs2_phase_vocoder", "fs2_pvoc_frames"], declared
    assert "fs2hip_pvoc.h" in _lib.EXTRA_HEADERS and _lib.HEADER_PVOC == HEADER
    assert "pvoc.hip" in g.HIP_SOURCES and len(_lib.SIGNATURES) == 71
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_PVOC[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+fs2_pvoc_frames\s*\(\s*int64_t\s+T\s*,\s*double\s+rate\s*\)", text)
    assert _lib.SIGNATURES_PVOC["fs2_pvoc_frames"] == (_lib._i64, [_lib._i64, _lib._d])
    assert re.search(r"\bint\s+fs2_phase_vocoder\s*\(\s*const\s+fs2_pvoc_desc\s*\*\s*d\s*,\s*fs2_stream_t\s+stream\s*\)", text)
    # the descriptor: the header's fields, in order, against the ctypes mirror
    body = re.search(r"typedef struct fs2_pvoc_desc \{(.*?)\} fs2_pvoc_desc;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = decl.replace("const", "").split()[0]
        for part in decl.split(","):
            name = re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1]
            fields.append((name, _lib._p if "*" in part else {"int": _lib._i, "int64_t": _lib._i64}[base]))
    assert fields == [(n, t) for n, t in _lib.PvocDesc._fields_], fields
    assert ctypes.sizeof(_lib.PvocDesc) == 6 * 8 + 4 * 4 + 3 * 8
    raw = open(HEADER).read()
    for name, val in (("FS2_PVOC_BLOCK", _lib.PVOC_BLOCK), ("FS2_PVOC_J_CAP", _lib.PVOC_J_CAP),
                      ("FS2_PVOC_B_MAX", _lib.PVOC_B_MAX)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", raw).group(1)) == val, name


def test_entry_rejects_bad_arguments_without_a_gpu():
    """The argument checks come before any launch, so they answer on a machine without a device."""
    import ctypes

    from fs2amd import _lib

    lib = _lib.load()
    p = 4096  # a non-null pointer that is never followed: every call below is refused first
    E, U = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    frames_host = (ctypes.c_int64 * 3)(10, 100, -3)
    rates_host = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

    def call(**kw):
        d = _lib.PvocDesc()
        d.spec, d.spec_row_stride, d.rates, d.recomb, d.recomb_row_stride, d.frames_out = p, 64, p, p, 128, p
        d.B, d.NB, d.T_max, d.J_max = 3, 5, 64, 128
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fs2_phase_vocoder(ctypes.byref(d), None)

    assert lib.fs2_phase_vocoder(None, None) == E
    for kw in (dict(spec=None), dict(rates=None), dict(recomb=None), dict(B=0), dict(B=-1), dict(NB=0), dict(T_max=0),
               dict(J_max=0), dict(spec_row_stride=63), dict(recomb_row_stride=127),
               # counts the host can see: 20, 128 (100 frames clamp to 64) and 0
               dict(frames=p, frames_host=ctypes.addressof(frames_host), rates_host=ctypes.addressof(rates_host),
                    J_max=127, recomb_row_stride=127),
               dict(rates_host=ctypes.addressof(rates_host), J_max=127, recomb_row_stride=127)):  # frames NULL: T_max each
        assert call(**kw) == E, kw
    assert call(B=65536) == U
    for kw in ({}, dict(B=65535)):
        assert _lib.pvoc_status(kw.get("B", 3), 5, 64, 128, 64, 128) == _lib.FS2_OK
    assert _lib.pvoc_status(65536, 5, 64, 128, 64, 128) == U and _lib.pvoc_status(3, 5, 64, 128, 63, 128) == E


def test_api_is_exported():
    import inspect

    import fs2amd
    from fs2amd import augment, ops

    for name in ("time_stretch", "pitch_shift", "augment_utterances"):
        assert name in fs2amd.__all__ and getattr(fs2amd, name) is getattr(augment, name)
    sig = inspect.signature(fs2amd.augment_utterances).parameters
    assert (sig["rates"].default, sig["n_steps"].default, sig["batch_size"].default) == ((), (), 16)
    assert callable(ops.phase_vocoder) and ops.pvoc_frames(64, 0.5) == 128
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.phase_vocoder(torch.zeros(1, 10, 8), None, [1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.time_stretch([np.zeros(1000, np.float32)], 0.9, stft=None, device="cpu")
    assert augment._suffix_rate(0.9) == "_ts0.90" and augment._suffix_steps(2) == "_ps+2"
    assert augment._suffix_steps(-3.0) == "_ps-3" and augment._suffix_steps(1.5) == "_ps+1.5"
