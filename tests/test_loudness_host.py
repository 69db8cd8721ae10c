"""Recursive filtering and BS.1770 loudness, host side (no GPU): the numpy restatement of
tests/_loudness.py against an np.longdouble direct recurrence, scipy.signal.sosfilt and the fixture
tests/golden/loudness_a.npz, the K-weighting table of the standard, the calibration tone, the gating
rules on hand-built rows, the size helpers and the C ABI of include/fs2hip_iir.h."""
import importlib.util
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch  # noqa: F401

import _loudness as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_iir.h")
H0 = 2205


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def rel_errors(sos, fs, seed):
    """(restatement, scipy) max |err| / max |y| against the longdouble recurrence on 2 s of int16 noise, and
    the restatement against scipy."""
    from scipy import signal

    x = R.noise_i16(2 * fs, seed)
    ref = R.sosfilt_ld(x, sos)
    m = float(np.abs(ref).max())
    y, _ = R.sosfilt(x, sos)
    sc = signal.sosfilt(sos, x.astype(np.float64))
    return float(np.abs(y - ref).max()) / m, float(np.abs(sc - ref).max()) / m, float(np.abs(y - sc).max()) / m


@pytest.mark.parametrize("fs", R.RATES)
def test_k_weighting_against_longdouble_and_scipy(fs):
    """2^-31 of the largest output: 1/128 of an f32 half-ulp at full scale, so y32 and every int16 result
    cannot see it. Measured: 6.4e-14 at 16000, 1.6e-13 at 22050, 3.9e-13 at 24000, 8.4e-13 at 44100 and
    1.8e-12 at 48000 (scipy's own sosfilt: 2e-14 .. 1.1e-13)."""
    mine, scipys, both = rel_errors(R.k_weighting(fs), fs, 1)
    print(f"k-weighting {fs}: restatement {mine:.2e}, scipy {scipys:.2e}, restatement against scipy {both:.2e}")
    assert mine <= 2.0 ** -31 and both <= 2.0 ** -31


@pytest.mark.parametrize("name", sorted(R.hostile_sos()))
def test_hostile_sections_against_longdouble_and_scipy(name):
    """2^-24. Measured: 5.9e-11 for butter(4, 20 Hz high-pass, 48 kHz), whose near-double pole at radius
    0.9976 makes the Q_i tables ill-conditioned (scipy: 4.9e-13); 3.7e-15 for the 300 - 3400 Hz band-pass at
    16 kHz; 4.3e-12 for the 50 Hz notch with poles at radius 0.9995."""
    sos, fs = R.hostile_sos()[name]
    if name == "notch50_r0999":
        assert min(abs(p) for p in np.roots(sos[0, 3:])) >= 0.999
    mine, scipys, both = rel_errors(sos, fs, 2)
    print(f"{name}: restatement {mine:.2e}, scipy {scipys:.2e}, restatement against scipy {both:.2e}")
    assert mine <= 2.0 ** -24 and both <= 2.0 ** -24


def test_k_weighting_reproduces_the_standards_table():
    from fs2amd.audio import k_weighting_sos, sos_tables
    from fs2amd import ops

    sos = k_weighting_sos(48000)
    table = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                      [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
    assert sos.dtype == np.float64 and sos.shape == (2, 6)
    assert np.abs(sos - table).max() <= 1e-13
    for fs in R.RATES:
        same_bits(k_weighting_sos(fs), R.k_weighting(fs))
        same_bits(sos_tables(R.k_weighting(fs)), R.tables(R.k_weighting(fs)))
    same_bits(ops.sos_tables(sos), R.tables(sos))
    assert R.tables(sos).shape == (2, R.TABLE_LEN)
    with pytest.raises(ValueError):
        k_weighting_sos(3000)
    with pytest.raises(ValueError):
        sos_tables([[1.0, 0.0, 0.0, 2.0, 0.0, 0.0]])


@pytest.mark.parametrize("fs", R.RATES)
def test_full_scale_997_hz_sine_reads_minus_3_01(fs):
    """Measured: -2.970 at 16 k, -2.981 at 22.05 k, -2.985 at 24 k, -3.008 at 44.1 k, -3.011 at 48 k: the drift
    below 44.1 k is the warping of the bilinear K-weighting design, not an error of the filter."""
    zbar, counts = R.measure(R.sine_row(fs), fs)
    lufs = R.lufs_of(zbar, np.int16)
    print(f"997 Hz at {fs}: {lufs:.4f} LUFS, blocks {counts}")
    assert counts[0] == counts[1] == counts[2] == 27
    assert abs(lufs - (-3.01)) <= 0.05


def test_loudness_against_the_longdouble_filter_with_plain_gating():
    """A 4 s burst-and-silence int16 row at 22050: <= 1e-8 LU, with no block within a relative 1e-6 of
    either gate (a gate flip is a different answer, not an error). Measured: 2e-12 LU."""
    fs = 22050
    x = R.speech_row(4 * fs, fs, 1)
    H = R.gate_hop(fs)
    ga = R.abs_gate(np.int16)
    zbar, counts = R.measure(x, fs)
    ref_y = R.sosfilt_ld(x, R.k_weighting(fs))
    ref_zbar, z, A, Rsel, mean_a = R.gate_plain(ref_y, H, np.longdouble(ga), np.longdouble(0.1))
    margin_abs = float(np.abs(z / np.longdouble(ga) - 1).min())
    margin_rel = float(np.abs(z[A] / (np.longdouble(0.1) * mean_a) - 1).min())
    assert margin_abs > 1e-6 and margin_rel > 1e-6, (margin_abs, margin_rel)
    assert counts == (len(z), int(A.sum()), int(Rsel.sum())) and 0 < counts[2] <= counts[1] < counts[0]
    diff = abs(10.0 * math.log10(zbar) - 10.0 * float(np.log10(ref_zbar)))
    print(f"loudness {R.lufs_of(zbar, np.int16):.4f} LUFS, {diff:.2e} LU from the longdouble reference, counts {counts}, "
          f"gate margins {margin_abs:.2e} {margin_rel:.2e}")
    assert diff <= 1e-8


def test_gating_cases():
    T = 4 * H0
    g = np.random.RandomState(9)
    ga = R.abs_gate(np.int16)
    for n, J in ((T - 1, 0), (T, 1), (T + H0 - 1, 1), (T + H0, 2)):
        y = g.standard_normal(n) * 500.0
        zbar, counts = R.gate(y, H0, ga)
        assert counts == (J, J, J) and R.blocks(n, H0) == J
        if J == 0:
            assert zbar == 0.0 and not np.signbit(zbar)
        else:  # against plain sums
            ref = R.gate_plain(y, H0, ga)[0]
            assert abs(zbar / ref - 1.0) < 1e-13
    # entirely under the absolute gate: -70 LUFS is a mean square of about 1.26e-7 * 32768^2 = 135 (int16 units)
    quiet = g.standard_normal(3 * 22050) * 3.0
    zbar, counts = R.gate(quiet, H0, ga)
    assert zbar == 0.0 and counts == (27, 0, 0)
    # the quiet second is over the absolute gate and under the relative one; the silent second under both
    fs = 8000
    x = R.two_level_row(fs)
    y, _ = R.sosfilt(x, R.k_weighting(fs))
    zbar, counts = R.gate(y, R.gate_hop(fs), ga)
    z = R.block_powers(y, R.gate_hop(fs))
    assert counts[0] == 27 and counts[2] < counts[1] < counts[0]
    A = z > ga
    assert (z[10:17] > ga).all() and (z[10:17] < 0.1 * z[A].mean()).all() and (z[20:] < ga).all()
    # what passes both: the loud second and the three blocks that overlap it
    assert counts == (27, 20, 10) and abs(zbar / z[:10].mean() - 1.0) < 1e-13
    # nothing measured: gain 1 and the flag; a measured row gets sqrt(target / zbar)
    r = R.normalize(np.zeros(3 * 22050, dtype=np.int16), 22050)
    assert r["gain"] == 1.0 and r["unmeasured"] == 1 and r["lufs"] == -math.inf and not r["q"].any()
    short = R.noise_i16(T - 1, 4)
    r = R.normalize(short, 22050)
    assert r["gain"] == 1.0 and r["unmeasured"] == 1 and r["counts"] == (0, 0, 0)
    same_bits(r["q"], short)
    r = R.normalize(x, fs, -23.0)
    assert r["unmeasured"] == 0 and r["gain"] == float(np.sqrt(np.float64(R.target_z(-23.0, np.int16)) / np.float64(zbar)))
    # re-measured after the gain: int16 rounding is the slack
    assert abs(R.lufs_of(R.measure(r["q"], fs)[0], np.int16) - (-23.0)) < 0.01
    # a gain that saturates, and a ceiling that lowers it
    loud = R.normalize(x, fs, -3.0)
    assert loud["clipped"] > 0 and loud["q"].max() == 32767 and loud["q"].min() == -32768
    capped = R.normalize(x, fs, -3.0, peak_ceiling=0.5)
    assert capped["clipped"] == 0 and capped["gain"] == 16384.0 / capped["peak"] < loud["gain"]
    assert np.abs(capped["q"].astype(np.int32)).max() == 16384
    low = R.normalize(x, fs, -40.0, peak_ceiling=0.99)  # a ceiling never raises the gain
    assert low["gain"] == R.normalize(x, fs, -40.0)["gain"]
    # ties to even
    rr = R.gain(np.array([1, 3, -1, -3, 5], dtype=np.int16), 4.0, 1.0)
    assert rr["gain"] == 0.5 and rr["q"].tolist() == [0, 2, 0, -2, 2]


def test_restatement_reproduces_the_fixture(fx):
    assert os.path.getsize(os.path.join(R.GOLDEN, "loudness_a.npz")) < 400 * 1024
    cases = R.fixture_cases()
    assert sorted(cases) == [str(n) for n in fx["names"]]
    for name, (x, fs) in cases.items():
        r = R.normalize(x, fs, -23.0)
        same_bits(np.float64(r["zbar"]), fx["zbar_" + name])
        same_bits(np.array(r["counts"], dtype=np.int32), fx["counts_" + name])
        same_bits(np.float64(r["gain"]), fx["gain_" + name])
        assert r["clipped"] == int(fx["clipped_" + name])
        same_bits(r["q"][:2000], fx["q_" + name])
    x, fs = cases["speech_i16_16000"]
    y, zf = R.sosfilt(x[:5000], R.k_weighting(fs))
    same_bits(y, fx["y_speech_i16_16000"])
    same_bits(zf, fx["zf_speech_i16_16000"])


def test_final_state_continues_the_filter():
    """zf of rule 6 is the state scipy reports, to rounding; fed back as zi it continues the row: the
    restatement of a row in two calls stays within the filter's own error of the row in one."""
    from scipy import signal

    sos = R.k_weighting(22050)
    x = R.noise_i16(9000, 6)
    for n in (1, 2, 64, 65, 4097):
        y, zf = R.sosfilt(x[:n], sos)
        ys, zs = signal.sosfilt(sos, x[:n].astype(np.float64), zi=np.zeros((2, 2)))
        assert np.abs(zf - zs).max() <= 1e-9 * max(1.0, np.abs(zs).max())
        y2, _ = R.sosfilt(x[n:], sos, zi=zf)
        whole, _ = R.sosfilt(x, sos)
        assert np.abs(np.concatenate([y, y2]) - whole).max() <= 1e-9 * np.abs(whole).max()
    zi = np.array([[1.5, -2.0], [0.25, 3.0]])
    y, zf = R.sosfilt(np.zeros(0, dtype=np.int16), sos, zi=zi)
    assert len(y) == 0
    same_bits(zf, zi)


def test_size_mirror_agrees_with_the_standalone_check():
    """tools/iir_sizes_check.py: the stand-alone host program over csrc/iir_sizes.h compares the header
    with the definitions and prints what the Python mirror has to give. The tool's own run builds it with
    ASan and UBSan (DESIGN 9.10 records that run); here the same program is built plainly, so that the
    comparison does not depend on a sanitizer runtime."""
    spec = importlib.util.spec_from_file_location("iir_sizes_check", os.path.join(REPO, "tools", "iir_sizes_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cxx = shutil.which("g++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler build() uses otherwise
    assert mod.check(cxx, sanitize=False) > 4000


def test_iir_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_IIR) == ["fs2_gain_int16", "fs2_iir_blocks", "fs2_iir_chunks",
                                                       "fs2_loudness_blocks", "fs2_loudness_gate",
                                                       "fs2_loudness_workspace_bytes", "fs2_sosfilt"], declared
    assert "fs2hip_iir.h" in _lib.EXTRA_HEADERS and _lib.HEADER_IIR == HEADER
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    ctype = {"int": _lib._i, "int64_t": _lib._i64, "double": _lib._d, "fs2_stream_t": _lib._p}
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_IIR[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m and ctype[m.group(1)] is res, name
        params = [p.strip() for p in m.group(2).split(",")]
        want = [_lib._p if "*" in p else ctype[p.split()[0]] for p in params]
        assert want == list(args), (name, params)
    raw = open(HEADER).read()
    for name, val in (("FS2_IIR_BLOCK", _lib.IIR_BLOCK), ("FS2_IIR_CHUNK", _lib.IIR_CHUNK), ("FS2_IIR_S_MAX", _lib.IIR_S_MAX),
                      ("FS2_IIR_TABLE_LEN", _lib.IIR_TABLE_LEN), ("FS2_IIR_B_MAX", _lib.IIR_B_MAX),
                      ("FS2_LOUD_H_MAX", _lib.LOUD_H_MAX)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", raw).group(1)) == val, name
    assert (R.BLOCK, R.CHUNK, R.TABLE_LEN, R.S_MAX) == (_lib.IIR_BLOCK, _lib.IIR_CHUNK, _lib.IIR_TABLE_LEN, _lib.IIR_S_MAX)
    from fs2amd import audio

    assert (audio.SOS_BLOCK, audio.SOS_TABLE_LEN) == (_lib.IIR_BLOCK, _lib.IIR_TABLE_LEN)
    assert "iir.hip" in __import__("__graft_entry__").HIP_SOURCES


def test_sizes_are_the_headers_formulas():
    from fs2amd import _lib

    lib = _lib.load()
    for n in (-3, 0, 1, 63, 64, 65, 16383, 16384, 16385, 220500):
        assert lib.fs2_iir_blocks(n) == _lib.iir_blocks(n) == (0 if n < 1 else -(-n // 64))
        assert lib.fs2_iir_chunks(n) == _lib.iir_chunks(n) == (0 if n < 1 else -(-n // 16384))
    for n, H in ((0, 2205), (8819, 2205), (8820, 2205), (11024, 2205), (11025, 2205), (220500, 2205), (5, 1), (3, 1)):
        assert lib.fs2_loudness_blocks(n, H) == _lib.loudness_blocks(n, H) == R.blocks(n, H)
        for B in (0, 1, 7, 64):
            assert lib.fs2_loudness_workspace_bytes(B, n, H) == _lib.loudness_workspace_bytes(B, n, H)
    assert lib.fs2_loudness_blocks(10, 0) == -1
    assert _lib.loudness_blocks(220500, 2205) == 97 and _lib.loudness_workspace_bytes(64, 220500, 2205) == 8 * 64 * (100 + 97 + 49)
    E, U, OK = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED, _lib.FS2_OK
    assert _lib.iir_status(1, 10, 8, 10) == OK and _lib.iir_status(1, 10, 9, 10) == U and _lib.iir_status(1, 10, 0, 10) == E
    assert _lib.iir_status(1, 10, 2, 9) == E and _lib.iir_status(65536, 10, 2, 10) == U
    assert _lib.loudness_status(1, 10, 32768) == OK and _lib.loudness_status(1, 10, 32769) == U
    assert _lib.loudness_status(1, 10, 0) == E and _lib.gain_status(65536, 1, 1) == U and _lib.gain_status(1, 5, 4) == E
