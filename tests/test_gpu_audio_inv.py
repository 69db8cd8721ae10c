"""fs2_stft / fs2_istft and Griffin-Lim on the GPU (include/fs2hip_audio_inv.h) against the float64
restatement of tests/_audio_inv.py and the reference's stored outputs (tests/golden/audio_inv_a.npz).

Parity bound: K x the reference's own statistic (its f32 CPU output against the same float64
restatement; ref_stats of the fixture), not a hard-coded number. K is the next power of two at or
above twice the largest kernel / reference ratio measured on the MI355X (DESIGN §9.1,
profiles/audio_inv/parity_ratios.txt: Z 0.99, M 0.55, W_inv 0.52, W_inv_edge 0.81, W_gl 0.44 -> K = 2);
it may not exceed 16. Both kernels sum in two levels; as single MFMA chains they measured Z 2.0 and
W_inv_edge 4.7.
"""
import numpy as np
import pytest
import torch

import _audio as A
import _audio_inv as AI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 2
assert K <= 16
ULP = 2.0 ** -24


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    from fs2amd import ops
    from fs2amd.audio import TacotronSTFT, window_sumsquare

    c = Ctx()
    c.z = z = AI.load_fixture()
    c.ref = z["ref_stats"]
    c.stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    c.fn = c.stft.stft_fn
    c.basis = c.fn.forward_basis.cpu().numpy().reshape(1026, 1024)
    c.inv = c.fn.inverse_basis.cpu().numpy().reshape(1026, 1024)
    c.audio_stats, c.r64 = A.fixture_stats(z, c.basis)  # M of the forward half, and its clipped mag64
    c.lens = torch.from_numpy(z["lens"])
    c.frames = [int(f) for f in z["frames"]]
    c.fr_t = torch.tensor(c.frames)
    c.n_max, c.T = int(c.lens.max()), max(c.frames)
    c.wav = torch.zeros(5, c.n_max)
    c.mag_b, c.ang_b = torch.zeros(5, 513, c.T), torch.zeros(5, 513, c.T)
    for b, w in enumerate(z["wavs"]):
        c.wav[b, :len(w)] = torch.from_numpy(w)
        c.mag_b[b, :, :c.frames[b]] = torch.from_numpy(z["mags"][b])
        c.ang_b[b, :, :c.frames[b]] = torch.from_numpy(z["angles_list"][b])
    c.wav, c.mag_b, c.ang_b = c.wav.to(DEV), c.mag_b.to(DEV), c.ang_b.to(DEV)
    c.ws = {t: window_sumsquare("hann", t) for t in set(c.frames) | {2, 33, 65, 66, 67, 130}}
    c.spec64 = [AI.transform64(w, c.basis) for w in z["wavs"]]
    c.tgt = c.mag_b + 0.25  # a target that is not 0 where the spectrum is
    c.st = ops.stft(c.wav, c.lens, stft=c.stft, mag_target=c.tgt)  # spec, mag and recomb in one launch
    c.recomb0 = torch.cat([c.mag_b * torch.cos(c.ang_b), c.mag_b * torch.sin(c.ang_b)], dim=1)
    c.inv_wav, c.inv_lens = ops.istft(c.recomb0, c.fr_t, stft=c.stft)
    c.inv64 = [AI.istft64(AI.recombine64(z["mags"][b], z["angles_list"][b]), c.inv, c.ws[t])
               for b, t in enumerate(c.frames)]
    torch.cuda.synchronize()
    return c


def _ratio(name, got, ref):
    print(f"{name}: kernel {got:.3e}  reference {ref:.3e}  ratio {got / ref:.3f}")
    return got / ref


def test_stft_parity_and_no_clipping(ctx):
    from fs2amd import ops

    c = ctx
    assert c.st.spec.shape == (5, 1026, 71) and c.st.mag.shape == (5, 513, 71) and c.st.recomb.shape == (5, 1026, 71)
    assert c.st.frames.tolist() == c.frames
    Z = max(AI.stat_Z(c.st.spec[b, :, :t].cpu().numpy(), c.spec64[b]) for b, t in enumerate(c.frames))
    # the magnitudes of the clipped signals: the M statistic of the forward half, like for like
    clipped = ops.stft(c.wav, c.lens, stft=c.stft, want=("mag",), clip=True)
    assert clipped.spec is None and clipped.recomb is None
    M = max(np.abs(clipped.mag[b, :, :t].cpu().numpy().T.astype(np.float64) - c.r64[b][0]).max()
            for b, t in enumerate(c.frames))
    rz, rm = _ratio("Z", Z, c.ref["Z"]), _ratio("M", M, c.audio_stats["M"])
    assert rz <= K and rm <= K
    # mag is |spec| of the same launch
    s = c.st.spec.double()
    assert (c.st.mag.double() - torch.hypot(s[:, :513], s[:, 513:])).abs().max() <= 2 * ULP * c.st.mag.max()
    # samples of 2.5 come back unclipped: the DC bin of a constant is the constant times the window's sum (512)
    x = torch.full((1, 4096), 2.5, device=DEV)
    assert abs(float(ops.stft(x, stft=c.stft).mag[0, 0, 8]) - 1280.0) < 1e-2
    assert abs(float(ops.stft(x, stft=c.stft, clip=True).mag[0, 0, 8]) - 512.0) < 1e-2
    assert float(c.wav.abs().max()) > 1.0


def test_projection_against_the_kernels_own_spectrum(ctx):
    from fs2amd import ops

    c = ctx
    spec, rec, m = c.st.spec.double().cpu(), c.st.recomb.double().cpu(), c.tgt.double().cpu()
    re, im = spec[:, :513], spec[:, 513:]
    a = torch.hypot(re, im)
    zero = a == 0
    worst = 0.0
    for b, t in enumerate(c.frames):
        sl = (b, slice(None), slice(0, t))
        an = torch.where(zero[sl], torch.ones_like(a[sl]), a[sl])
        want_re = torch.where(zero[sl], m[sl], m[sl] * re[sl] / an)
        want_im = torch.where(zero[sl], torch.zeros_like(an), m[sl] * im[sl] / an)
        err = torch.maximum((rec[b, :513, :t] - want_re).abs(), (rec[b, 513:, :t] - want_im).abs()) / m[sl]
        worst = max(worst, float(err.max()))
        # exactly (m, 0) where the spectrum is (0, 0)
        assert torch.equal(rec[b, :513, :t][zero[sl]], m[sl][zero[sl]]) and not rec[b, 513:, :t][zero[sl]].any()
        assert not rec[b, :, t:].any()
    print(f"projection: worst |recomb - m z/|z|| / m = {worst / ULP:.2f} x 2^-24 (bound 8)")
    assert worst <= 8 * ULP  # five f32 roundings, doubled
    assert zero[4, :, :71].all(dim=0).any(), "utterance 4 has frames of digital silence"
    # scale-robust: 2^-100 times utterance 3 (exact scaling, far above the denormals) projects alike
    n, t = int(c.lens[3]), c.frames[3]
    small = ops.stft(c.wav[3:4, :n] * 2.0 ** -100, stft=c.stft, mag_target=c.tgt[3:4, :, :t].contiguous(), want=())
    assert small.spec is None and small.mag is None
    d = (small.recomb[0].double().cpu() - rec[3, :, :t]).abs() / torch.cat([m[3, :, :t], m[3, :, :t]])
    print(f"projection of the 2^-100 signal: {float(d.max()) / ULP:.2f} x 2^-24 from the unscaled one")
    assert float(d.max()) <= 8 * ULP


def test_istft_parity(ctx):
    from fs2amd import ops

    c = ctx
    assert c.inv_wav.shape == (5, 256 * 70) and c.inv_lens.tolist() == [256 * (t - 1) for t in c.frames]
    W = Wedge = Wref = 0.0
    for b, t in enumerate(c.frames):
        got = c.inv_wav[b, :256 * (t - 1)].cpu().numpy()
        W, Wedge = max(W, AI.stat_W(got, c.inv64[b])), max(Wedge, AI.stat_W_edge(got, c.inv64[b]))
        Wref = max(Wref, AI.stat_W(got, c.z["ref_inverse_list"][b].astype(np.float64)))
        assert not c.inv_wav[b, 256 * (t - 1):].any()
    r = [_ratio("W_inv", W, c.ref["W_inv"]), _ratio("W_inv_edge", Wedge, c.ref["W_inv_edge"])]
    assert max(r) <= K
    assert Wref <= (K + 1) * c.ref["W_inv"]  # the reference's values, both ways round
    # random recomb: no output, the shortest output, 1-3 frames past a tile boundary, two tiles and more
    Ts = [1, 2, 65, 66, 67, 130]
    g = torch.Generator().manual_seed(7)
    rc = torch.randn(len(Ts), 1026, 130, generator=g)
    wav, lens = ops.istft(rc.to(DEV), torch.tensor(Ts), stft=c.stft)
    assert lens.tolist() == [256 * (t - 1) for t in Ts] and wav.shape == (6, 256 * 129)
    Wr = 0.0
    for b, t in enumerate(Ts):
        assert not wav[b, 256 * (t - 1):].any()
        if t > 1:
            w64 = AI.istft64(rc[b, :, :t].numpy(), c.inv, c.ws[t])
            Wr = max(Wr, AI.stat_W(wav[b, :256 * (t - 1)].cpu().numpy(), w64))
    assert _ratio("W_inv(random)", Wr, c.ref["W_inv"]) <= K


def _nan_padded(t, pad_last, pad_stride):
    """t's values in a view with NaN beyond its last dimension and a wider row stride."""
    big = torch.full(t.shape[:-1] + (t.shape[-1] + pad_last + pad_stride,), float("nan"), device=t.device)
    big[..., :t.shape[-1]] = t
    return big[..., :t.shape[-1] + pad_last]


def test_ragged_batches_are_bit_exact(ctx):
    from fs2amd import ops

    c = ctx
    GL = 3
    idx = [1, 2, 3, 4]  # Griffin-Lim needs T >= 4
    fr4 = c.fr_t[idx]
    gl_wav, gl_lens = ops.griffin_lim(c.mag_b[idx], fr4, stft=c.stft, n_iters=GL, angles=c.ang_b[idx])
    assert gl_lens.tolist() == [256 * (c.frames[b] - 1) for b in idx]
    full = (c.st.spec, c.st.mag, c.st.recomb)
    for b in range(5):  # each utterance alone (B = 1, n_max = lens, T = frames)
        n, t = int(c.lens[b]), c.frames[b]
        one = ops.stft(c.wav[b:b + 1, :n].contiguous(), stft=c.stft, mag_target=c.tgt[b:b + 1, :, :t].contiguous())
        assert one.frames.tolist() == [t]
        for got, want in zip(one[:3], full):
            assert torch.equal(got[0], want[b, :, :t]), b
        w1, l1 = ops.istft(c.recomb0[b:b + 1, :, :t].contiguous(), stft=c.stft)
        assert l1.tolist() == [256 * (t - 1)] and torch.equal(w1[0], c.inv_wav[b, :256 * (t - 1)]), b
        if t >= 4:
            g1, _ = ops.griffin_lim(c.mag_b[b:b + 1, :, :t].contiguous(), stft=c.stft, n_iters=GL,
                                    angles=c.ang_b[b:b + 1, :, :t].contiguous())
            k = idx.index(b)
            assert torch.equal(g1[0], gl_wav[k, :256 * (t - 1)]) and not gl_wav[k, 256 * (t - 1):].any(), b
    # reversed batch order
    rev = ops.stft(c.wav.flip(0).contiguous(), c.lens.flip(0), stft=c.stft, mag_target=c.tgt.flip(0).contiguous())
    for got, want in zip(rev[:3], full):
        assert torch.equal(got.flip(0), want)
    wr, lr = ops.istft(c.recomb0.flip(0).contiguous(), c.fr_t.flip(0), stft=c.stft)
    assert torch.equal(wr.flip(0), c.inv_wav) and torch.equal(lr.flip(0), c.inv_lens)
    gr, _ = ops.griffin_lim(c.mag_b[idx].flip(0).contiguous(), fr4.flip(0), stft=c.stft, n_iters=GL,
                            angles=c.ang_b[idx].flip(0).contiguous())
    assert torch.equal(gr.flip(0), gl_wav)
    # NaN past every length, longer rows and a row stride wider than the row
    wav_p = _nan_padded(c.wav, 1000, 77)
    for b in range(5):
        wav_p[b, int(c.lens[b]):] = float("nan")
    tgt_p = _nan_padded(c.tgt, 6, 3)
    for b, t in enumerate(c.frames):
        tgt_p[b, :, t:] = float("nan")
    assert wav_p.stride(0) > wav_p.shape[1] and tgt_p.stride(1) > tgt_p.shape[2]
    pad = ops.stft(wav_p, c.lens, stft=c.stft, mag_target=tgt_p, T_out=74)
    for got, want in zip(pad[:3], full):
        assert torch.equal(got[:, :, :71], want) and not got[:, :, 71:].any()
    rec_p, mag_p, ang_p = _nan_padded(c.recomb0, 6, 3), _nan_padded(c.mag_b, 6, 3), _nan_padded(c.ang_b, 6, 3)
    for b, t in enumerate(c.frames):
        rec_p[b, :, t:] = mag_p[b, :, t:] = ang_p[b, :, t:] = float("nan")
    wp, lp = ops.istft(rec_p, c.fr_t, stft=c.stft, n_out_max=256 * 70 + 300)
    assert torch.equal(wp[:, :256 * 70], c.inv_wav) and not wp[:, 256 * 70:].any() and torch.equal(lp, c.inv_lens)
    gp, lp = ops.griffin_lim(mag_p[1:5], fr4, stft=c.stft, n_iters=GL, angles=ang_p[1:5])  # views: the wide stride stays
    assert gp.shape == (4, 256 * 76) and torch.equal(gp[:, :256 * 70], gl_wav) and not gp[:, 256 * 70:].any()
    assert torch.equal(lp, gl_lens)


def test_griffin_lim_parity_and_convergence(ctx):
    from fs2amd import ops

    c = ctx
    idx = [1, 2, 3, 4]
    wav, lens = ops.griffin_lim(c.mag_b[idx], c.fr_t[idx], stft=c.stft, n_iters=AI.GL_ITERS, angles=c.ang_b[idx])
    first, _ = ops.griffin_lim(c.mag_b[idx], c.fr_t[idx], stft=c.stft, n_iters=0, angles=c.ang_b[idx])
    mag_n = ops.stft(wav, lens, stft=c.stft, want=("mag",)).mag.double().cpu()
    mag_0 = ops.stft(first, lens, stft=c.stft, want=("mag",)).mag.double().cpu()
    W = Wref = 0.0
    for k, b in enumerate(idx):
        t = c.frames[b]
        g64 = AI.gl64(c.z["mags"][b], c.z["angles_list"][b], AI.GL_ITERS, c.basis, c.inv, c.ws[t])
        got = wav[k, :256 * (t - 1)].cpu().numpy()
        W = max(W, AI.stat_W(got, g64))
        Wref = max(Wref, AI.stat_W(got, c.z["ref_gl_list"][b].astype(np.float64)))
        m = c.mag_b[b, :, :t].double().cpu()
        sc_n, sc_0 = float((mag_n[k, :, :t] - m).norm() / m.norm()), float((mag_0[k, :, :t] - m).norm() / m.norm())
        print(f"utterance {b}: spectral convergence {sc_0:.4f} -> {sc_n:.4f} after {AI.GL_ITERS} iterations")
        assert sc_n < sc_0, b
    assert _ratio("W_gl", W, c.ref["W_gl"]) <= K
    assert Wref <= (K + 1) * c.ref["W_gl"]
    with pytest.raises(ValueError, match="at least 4 frames"):
        ops.griffin_lim(c.mag_b[:2], c.fr_t[:2], stft=c.stft, n_iters=1, angles=c.ang_b[:2])


def test_drop_in_surface(ctx, tmp_path):
    from fs2amd.audio import griffin_lim, inv_mel_spec, mel_to_wav

    c = ctx
    # transform / inverse / forward of one utterance, as the reference is called
    n, t = int(c.lens[2]), c.frames[2]
    mag, phase = c.fn.transform(c.wav[2:3, :n])
    assert mag.shape == phase.shape == (1, 513, t) and torch.equal(mag[0], c.st.mag[2, :, :t])
    big = torch.from_numpy(np.hypot(c.spec64[2][:513], c.spec64[2][513:]) > 1e-2)
    d = torch.angle(torch.exp(1j * (phase[0].cpu() - torch.from_numpy(c.z["phase_u2"]))))
    # a phase moves by |dz| / |z|: the two spectra are within K Z and Z of float64; each atan2 adds 2 ulp at pi
    assert float((d.abs() * mag[0].cpu() - 16 * ULP * mag[0].cpu())[big].max()) <= (K + 1) * c.ref["Z"]
    for b, tb in enumerate(c.frames):
        out = c.fn.inverse(c.mag_b[b:b + 1, :, :tb].contiguous(), c.ang_b[b:b + 1, :, :tb].contiguous())
        assert out.shape == (1, 1, 256 * (tb - 1)) and torch.equal(out[0, 0], c.inv_wav[b, :256 * (tb - 1)])
    assert c.fn.inverse(c.mag_b[:1, :, :1].contiguous(), c.ang_b[:1, :, :1].contiguous()).shape == (1, 1, 0)
    rec = c.fn(c.wav[2:3, :n])
    assert rec.shape == (1, 1, 256 * (t - 1)) and torch.equal(rec, c.fn.inverse(c.fn.magnitude, c.fn.phase))
    err = float((rec[0, 0] - c.wav[2, :256 * (t - 1)]).abs().max() / c.wav[2, :n].abs().max())
    print(f"forward(x) against x: {err:.3e} of the peak")
    sig = griffin_lim(c.mag_b[3:4, :, :34].contiguous(), c.fn, 2, angles=c.ang_b[3:4, :, :34].contiguous())
    assert sig.shape == (1, 256 * 33)
    # inv_mel_spec: Griffin-Lim on its own spec_from_mel (last frame dropped), against float64
    mel = torch.from_numpy(np.ascontiguousarray(c.z["ref_mel_list"][3].T)).to(DEV)  # [80, 34]
    ang = c.ang_b[3:4, :, :33].contiguous()
    path = tmp_path / "a.wav"
    audio = inv_mel_spec(mel, str(path), c.stft, AI.GL_ITERS, angles=ang)
    assert isinstance(audio, np.ndarray) and audio.dtype == np.float32 and audio.shape == (256 * 32,)
    assert np.array_equal(inv_mel_spec(mel, None, c.stft, AI.GL_ITERS, angles=ang), audio)
    raw = path.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and np.array_equal(np.frombuffer(raw[-4 * len(audio):], "<f4"), audio)
    g64 = AI.gl64(c.z["spec_from_mel"], ang[0].cpu().numpy(), AI.GL_ITERS, c.basis, c.inv, c.ws[33])
    assert _ratio("W_gl(inv_mel_spec)", AI.stat_W(audio, g64), c.ref["W_gl"]) <= K
    # mel_to_wav: the same for a ragged batch in the model's layout
    mels = torch.zeros(2, 34, 80, device=DEV)
    mels[0], mels[1, :5] = mel.t(), torch.from_numpy(c.z["ref_mel_list"][1]).to(DEV)
    angs = torch.zeros(2, 513, 33, device=DEV)
    angs[0], angs[1, :, :4] = ang[0], c.ang_b[1, :, :4]
    wav, lens = mel_to_wav(mels, [34, 5], c.stft, AI.GL_ITERS, angles=angs)
    assert wav.shape == (2, 256 * 32) and lens.tolist() == [256 * 32, 256 * 3] and not wav[1, 256 * 3:].any()
    assert np.array_equal(wav[0].cpu().numpy(), audio)
    one = inv_mel_spec(mels[1, :5].t(), None, c.stft, AI.GL_ITERS, angles=angs[1:2, :, :4].contiguous())
    assert np.array_equal(wav[1, :256 * 3].cpu().numpy(), one)


def test_library_ops_and_graph_replay(ctx):
    import fs2amd.library  # noqa: F401
    from fs2amd import ops

    c = ctx
    spec, mag, frames = torch.ops.fs2.stft(c.wav, c.lens.to(DEV), c.fn.forward_basis, 71, 256, 1024, False)
    assert torch.equal(spec, c.st.spec) and torch.equal(mag, c.st.mag) and frames.tolist() == c.frames
    wav, lens = torch.ops.fs2.istft(c.recomb0, c.fr_t.to(DEV), c.fn.inverse_packed, c.fn.wsum_table, 256 * 70, 256, 1024)
    assert torch.equal(wav, c.inv_wav) and torch.equal(lens, c.inv_lens)
    with pytest.raises(RuntimeError, match=r"fs2 status 1 "):  # FS2_EINVAL: the host sees 71 frames
        ops.stft(c.wav, c.lens, stft=c.stft, T_out=70)
    with pytest.raises(RuntimeError, match=r"fs2 status 1 "):  # 256 * 70 samples
        ops.istft(c.recomb0, c.fr_t, stft=c.stft, n_out_max=256 * 70 - 1)

    # one captured Griffin-Lim (B = 2, T = 5, 2 iterations) replayed equals the eager bits, also for new contents
    mag2, ang2 = c.mag_b[1:3, :, :5].clone(), c.ang_b[1:3, :, :5].clone()
    fr = torch.tensor([5, 5], device=DEV)
    out = (torch.empty(2, 1024, device=DEV), torch.empty(2, device=DEV, dtype=torch.int64))
    ws = torch.empty(2, 1026, 5, device=DEV)
    kw = dict(stft=c.stft, n_iters=2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.griffin_lim(mag2, fr, angles=ang2, out=out, workspace=ws, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.griffin_lim(mag2, fr, angles=ang2, out=out, workspace=ws, **kw)
    for mags, angs, frs in ((c.mag_b[1:3, :, :5], c.ang_b[1:3, :, :5], [5, 5]), (c.mag_b[3:5, :, 2:7], c.ang_b[3:5, :, 9:14], [4, 5])):
        mag2.copy_(mags)
        ang2.copy_(angs)
        fr.copy_(torch.tensor(frs, device=DEV))
        g.replay()
        torch.cuda.synchronize()
        eager, elens = ops.griffin_lim(mag2.clone(), torch.tensor(frs), angles=ang2.clone(), **kw)
        assert torch.equal(out[0], eager) and torch.equal(out[1], elens) and elens.tolist() == [256 * (f - 1) for f in frs]
        assert float(eager.abs().max()) > 0
