"""Inverse STFT and Griffin-Lim, host side (no GPU): the float64 yardstick of test_gpu_audio_inv.py
against the reference's own stored outputs, the window sum and the inverse basis against the
reference-built ones, the C ABI of include/fs2hip_audio_inv.h, and the torch.library registration."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _audio_inv as AI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_audio_inv.h")


@pytest.fixture(scope="module")
def fx():
    return AI.load_fixture()


@pytest.fixture(scope="module")
def stft():
    from fs2amd.audio import TacotronSTFT

    return TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0)


def test_float64_yardstick_agrees_with_the_reference_outputs(fx, stft):
    """One inverse: the reference's f32 result is within 1e-6 of the peak of the restatement (the
    issue's figure; asserted at 5e-6), a whole 8-iteration Griffin-Lim run within 1e-5 (5e-5). The
    stored ref_stats are these very figures."""
    from fs2amd.audio import window_sumsquare

    basis = stft.forward_basis.numpy().reshape(1026, 1024)
    inv = stft.stft_fn.inverse_basis.numpy().reshape(1026, 1024)
    W_inv = W_edge = W_gl = 0.0
    for b, t in enumerate(fx["frames"]):
        ws = window_sumsquare("hann", int(t))
        w64 = AI.istft64(AI.recombine64(fx["mags"][b], fx["angles_list"][b]), inv, ws)
        assert w64.shape == fx["ref_inverse_list"][b].shape == (256 * (t - 1),)
        W_inv = max(W_inv, AI.stat_W(fx["ref_inverse_list"][b], w64))
        W_edge = max(W_edge, AI.stat_W_edge(fx["ref_inverse_list"][b], w64))
        if t >= 4:
            trace = []
            g64 = AI.gl64(fx["mags"][b], fx["angles_list"][b], AI.GL_ITERS, basis, inv, ws, trace)
            W_gl = max(W_gl, AI.stat_W(fx["ref_gl_list"][b], g64))
            assert trace[-1] < trace[0], (b, trace)  # the iteration converges on these magnitudes
    print(f"reference vs float64: W_inv {W_inv:.3e} W_inv_edge {W_edge:.3e} W_gl {W_gl:.3e}; stored {fx['ref_stats']}")
    assert W_inv < 5e-6 and W_edge < 5e-6 and W_gl < 5e-5
    for k, v in (("W_inv", W_inv), ("W_inv_edge", W_edge), ("W_gl", W_gl)):
        assert 0.5 * fx["ref_stats"][k] <= v <= 2 * fx["ref_stats"][k], k  # a LAPACK's pinv may differ in the last bits
    assert 0 < fx["ref_stats"]["Z"] < 5e-4
    # the fixture has what the exact GPU checks need: frames of digital silence in utterance 4
    assert (fx["mags"][4] == 0).all(axis=0).any()
    # utterance 2's stored phase is atan2 of the restated spectrum wherever the bin is not tiny
    s64 = AI.transform64(fx["wavs"][2], basis)
    big = np.hypot(s64[:513], s64[513:]) > 1e-2
    d = np.angle(np.exp(1j * (fx["phase_u2"] - np.arctan2(s64[513:], s64[:513]))))
    assert fx["phase_u2"].shape == (513, 5) and np.abs(d[big]).max() < 1e-3


def test_window_sumsquare_and_edge_table_bit_for_bit(fx):
    from fs2amd.audio import window_sum_from_table, window_sumsquare, wsum_edge_table

    table = wsum_edge_table()
    assert table.shape == (16, 256) and table.dtype == np.float32 and not table[0].any()
    for t in AI.WSUM_T:
        want = fx[f"wsum_{t}"]
        got = window_sumsquare("hann", t, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
        assert got.dtype == np.float32 and got.shape == want.shape == (1024 + 256 * (t - 1),)
        assert np.array_equal(got, want), t
        assert np.array_equal(window_sum_from_table(table, t), want), t
        if t >= 2:
            assert want[512:len(want) - 512].min() >= 1.25  # the reference's `> tiny` test is always true there
    assert np.abs(fx["wsum_71"][2048:-2048] - 1.5).max() <= 2.0 ** -22  # 1.5 in the interior, to the f32 accumulator


def test_inverse_basis_rows_and_packing(fx, stft):
    from fs2amd import _lib
    from fs2amd.audio import pack_inverse_basis

    inv = stft.stft_fn.inverse_basis
    assert inv.shape == (1026, 1, 1024) and inv.dtype == torch.float32
    rows = inv.numpy().reshape(1026, 1024)[fx["inv_row_ids"]]
    assert np.abs(fx["inv_rows"]).max() < 4.9e-4
    assert np.abs(rows.astype(np.float64) - fx["inv_rows"]).max() <= 1.2e-10  # 2 ulp at the largest entry
    packed = stft.stft_fn.inverse_packed
    assert packed.shape == (129, 4, 256, 2, 4) and packed.is_contiguous() and packed.numel() == 4 * _lib.ISTFT_KPAD * 256
    assert torch.equal(packed, pack_inverse_basis(inv))
    flat, m = packed.reshape(-1), inv.reshape(1026, 1024)
    g = torch.Generator().manual_seed(3)
    for _ in range(200):
        gi, q, r, h, e = (int(torch.randint(0, n, (1,), generator=g)) for n in (129, 4, 256, 2, 4))
        c = 8 * gi + 2 * e + h
        want = m[c, 256 * q + r] if c < 1026 else 0.0
        assert flat[(((gi * 4 + q) * 256 + r) * 2 + h) * 4 + e] == want
    assert stft.stft_fn.wsum_table.shape == (16, 256)


def test_state_dict_keys_unchanged(stft):
    from fs2amd.audio import TacotronSTFT

    fresh = TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0)
    assert set(fresh.state_dict()) == {"stft_fn.forward_basis", "mel_basis"}
    assert "inverse_basis" not in dict(fresh.stft_fn.named_buffers())  # built on first use only
    _ = stft.stft_fn.inverse_basis
    assert set(stft.state_dict()) == {"stft_fn.forward_basis", "mel_basis"}
    assert {"inverse_basis", "inverse_packed", "wsum_table"} <= set(dict(stft.stft_fn.named_buffers()))
    fresh.load_state_dict(stft.state_dict())


def test_lens_out_formula():
    from fs2amd import ops

    assert [ops.istft_len(t) for t in (0, 1, 2, 3, 71)] == [0, 0, 256, 512, 17920]
    assert ops.istft_len(torch.tensor([0, 1, 2, 71])).tolist() == [0, 0, 256, 17920]
    # a Griffin-Lim signal of T frames has T frames again
    assert all(ops.mel_frames(ops.istft_len(t)) == t for t in range(4, 80))
    assert ops.mel_frames(ops.istft_len(3)) == 0 and ops.GRIFFIN_LIM_MIN_FRAMES == 4


def test_audio_inv_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_AUDIO_INV) == ["fs2_istft", "fs2_stft"], declared
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_PROSODY) | set(_lib.SIGNATURES_AUDIO))
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES_AUDIO_INV[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "fs2hip_audio_inv.h" in _lib.EXTRA_HEADERS  # the build id covers the header


@pytest.mark.parametrize("cname, mirror", [("fs2_stft_desc", "StftDesc"), ("fs2_istft_desc", "IstftDesc")])
def test_desc_layouts_match_header(tmp_path, cname, mirror):
    from fs2amd import _lib

    cls = getattr(_lib, mirror)
    names = [f[0] for f in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fs2hip_audio_inv.h"\nint main(void){' + "".join(
        f'printf("{n} %zu\\n", offsetof({cname}, {n}));' for n in names) + \
        f'printf("size %zu\\n", sizeof({cname})); printf("kpad %d\\n", FS2_ISTFT_KPAD); ' \
        'printf("packed %d\\n", FS2_ISTFT_PACKED_ELEMS); printf("wsum %d\\n", FS2_ISTFT_WSUM_ELEMS); }\n'
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")],
                   check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert got.pop("size") == ctypes.sizeof(cls) and got.pop("kpad") == _lib.ISTFT_KPAD == 1032
    assert got.pop("packed") == 4 * 1032 * 256 and got.pop("wsum") == 16 * 256
    assert got == {n: getattr(cls, n).offset for n in names}


def test_entries_reject_bad_descriptors_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    EINVAL, EUNS = _lib.FS2_EINVAL, _lib.FS2_EUNSUPPORTED
    assert lib.fs2_stft(None, None) == EINVAL and lib.fs2_istft(None, None) == EINVAL

    d = _lib.StftDesc()
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL
    d.wav, d.basis = 4096, 4096
    d.B, d.n_max, d.T_out, d.wav_row_stride = 2, 1024, 5, 1024
    d.n_fft, d.hop, d.win = 1024, 256, 1024
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL  # no output at all
    d.spec = 4096
    d.mag_target, d.mag_row_stride = 4096, 5
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL  # mag_target without recomb
    d.mag_target, d.recomb = None, 4096
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL  # recomb without mag_target
    d.mag_target, d.mag_row_stride = 4096, 4
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL  # a stride smaller than the row
    d.mag_row_stride = 5
    d.n_fft, d.win = 512, 512
    assert lib.fs2_stft(ctypes.byref(d), None) == EUNS
    d.n_fft, d.win, d.hop = 1024, 1024, 128
    assert lib.fs2_stft(ctypes.byref(d), None) == EUNS
    d.hop, d.T_out, d.mag_row_stride = 256, 4, 4  # lens NULL: every row has 1 + 1024 / 256 = 5 frames
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL
    host = (ctypes.c_int64 * 2)(513, 1279)
    d.lens, d.lens_host = 4096, ctypes.cast(host, ctypes.c_void_p)  # frames 3 and 5
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL
    d.T_out, d.mag_row_stride, d.wav_row_stride = 5, 5, 1000
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL
    d.wav_row_stride, d.B = 1024, 0
    assert lib.fs2_stft(ctypes.byref(d), None) == EINVAL

    e = _lib.IstftDesc()
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL
    for k in ("recomb", "inv_packed", "wsum_table", "wav"):
        setattr(e, k, 4096)
    e.B, e.T_in, e.n_out_max, e.recomb_row_stride, e.wav_row_stride = 2, 5, 1024, 5, 1024
    e.n_fft, e.hop, e.win = 1024, 256, 512
    assert lib.fs2_istft(ctypes.byref(e), None) == EUNS
    e.win, e.n_out_max, e.wav_row_stride = 1024, 1023, 1023  # frames NULL: 256 * (5 - 1) samples each
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL
    fhost = (ctypes.c_int64 * 2)(3, 5)
    e.frames, e.frames_host = 4096, ctypes.cast(fhost, ctypes.c_void_p)
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL
    e.n_out_max, e.wav_row_stride, e.recomb_row_stride = 1024, 1024, 4
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL
    e.recomb_row_stride, e.wav_row_stride = 5, 1000
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL
    e.wav_row_stride, e.wsum_table = 1024, None
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL
    e.wsum_table, e.T_in = 4096, 0
    assert lib.fs2_istft(ctypes.byref(e), None) == EINVAL


def test_griffin_lim_needs_four_frames_and_a_gpu(stft):
    import fs2amd
    from fs2amd import ops

    for name in ("STFT", "griffin_lim", "inv_mel_spec", "mel_to_wav", "window_sumsquare"):
        assert hasattr(fs2amd, name) and name in fs2amd.__all__
    with pytest.raises(ValueError, match="at least 4 frames"):
        fs2amd.griffin_lim(torch.ones(1, 513, 3), stft.stft_fn, 2)
    with pytest.raises(ValueError, match="at least 4 frames"):
        ops.griffin_lim(torch.ones(2, 513, 6), torch.tensor([6, 3]), stft=stft, n_iters=2)
    with pytest.raises(ValueError, match="mel_lens >= 5"):
        fs2amd.mel_to_wav(torch.zeros(2, 9, 80), [9, 4], stft)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.griffin_lim(torch.ones(1, 513, 4), stft.stft_fn, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft.stft_fn.transform(torch.zeros(1, 2048))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft.stft_fn.inverse(torch.ones(1, 513, 4), torch.zeros(1, 513, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs2amd.inv_mel_spec(torch.zeros(80, 9), None, stft, 2)
    assert stft.stft_fn.inverse(torch.ones(1, 513, 1), torch.zeros(1, 513, 1)).shape == (1, 1, 0)


def test_spec_from_mel_is_the_reference_arithmetic(fx, stft):
    from fs2amd.audio import spec_from_mel

    got = spec_from_mel(torch.from_numpy(np.ascontiguousarray(fx["ref_mel_list"][3].T)), stft)
    assert got.shape == (1, 513, 34)
    want = fx["spec_from_mel"]
    assert want.shape == (513, 33)
    # the same f32 product of the same operands; a BLAS may order the 80 terms differently
    assert np.abs(got[0, :, :-1].numpy() - want).max() <= 80 * 2.0 ** -24 * np.abs(want).max()


def test_ops_registered_with_fake_shapes():
    import fs2amd.library as lib
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert lib.OPS[-2:] == ("stft", "istft") and all(hasattr(torch.ops.fs2, n) for n in lib.OPS)
    with FakeTensorMode():
        wav = torch.empty(3, 5000, device="cuda")
        lens = torch.empty(3, device="cuda", dtype=torch.int64)
        spec, mag, fr = torch.ops.fs2.stft(wav, lens, torch.empty(1026, 1, 1024, device="cuda"), 20, 256, 1024, False)
        assert spec.shape == (3, 1026, 20) and mag.shape == (3, 513, 20) and spec.dtype == mag.dtype == torch.float32
        assert fr.shape == (3,) and fr.dtype == torch.int64
        out, n = torch.ops.fs2.istft(spec, fr, torch.empty(129, 4, 256, 2, 4, device="cuda"),
                                     torch.empty(16, 256, device="cuda"), 19 * 256, 256, 1024)
        assert out.shape == (3, 19 * 256) and out.dtype == torch.float32 and n.shape == (3,) and n.dtype == torch.int64
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.fs2.stft(torch.zeros(1, 2048), None, torch.zeros(1026, 1, 1024), 9, 256, 1024, False)
