#!/usr/bin/env python3
"""Generate tests/golden/audio_inv_a.npz by running the REFERENCE's audio/ package on the CPU.

Runs only where the reference tree is mounted (FS2_REFERENCE, default /root/reference); only the
.npz travels. The accommodations are those of gen_golden_audio.py (librosa stand-ins,
``torch.Tensor.cuda`` as the identity), plus, for the duration of single calls:

* ``np.random.rand`` returns the stored uniform draws, so that the reference's griffin_lim starts
  from the stored angles;
* ``torch.nn.functional.conv1d`` is wrapped to keep its result: STFT.transform returns magnitude and
  phase only, and the Z statistic needs the reference's own f32 spectrum;
* ``inv_mel_spec`` is run with ``_stft._stft_fn = _stft.stft_fn`` (the attribute it asks for does not
  exist) and with ``audio.tools.griffin_lim`` / ``write`` replaced by recorders: what is stored is the
  magnitudes argument it hands to griffin_lim (``spec_from_mel`` without its last frame).

Inputs: the five utterances of audio_a.npz (3, 5, 5, 34 and 71 frames) with the reference's own
stored magnitudes as targets. Stored, all f32 and ragged (concatenated):

  angles            initial phases per utterance [513, T], np.angle(exp(2j pi u)) as the reference
  ref_inverse       STFT.inverse(mag, angles), 256 (T - 1) samples, all five
  ref_gl            griffin_lim(mag, stft_fn, 8) from those angles, utterances 1-4 (T >= 4)
  wsum_<T>          window_sumsquare for T in 1..6 and 71
  inv_rows          9 rows (inv_row_ids) of inverse_basis [1026, 1024]
  phase_u2          STFT.transform's phase of utterance 2 (not clipped), [513, 5]
  spec_from_mel     inv_mel_spec's magnitudes for the mel of utterance 3, [513, 33]
  ref_stats         W_inv, W_inv_edge, W_gl, Z: the reference's f32 results against the float64
                    restatement of tests/_audio_inv.py (printed)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_audio_inv.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_audio as G  # noqa: E402  (sets sys.path for fs2amd and tests/)

import _audio_inv as AI  # noqa: E402
from _npz_parts import save_npz_parts  # noqa: E402

from fs2amd.audio import window_sumsquare  # noqa: E402


def main():
    ref_stft, ref_tools = G.import_reference_audio()
    import audio.audio_processing as ref_ap

    z = AI.A.load_fixture()
    frames = [int(f) for f in z["frames"]]
    mags = [np.ascontiguousarray(m.T) for m in z["ref_mag_list"]]  # [513, T]
    rng = np.random.default_rng(20261)
    uniform = [rng.random((1, AI.N_BINS, t)) for t in frames]
    angles = [np.angle(np.exp(2j * np.pi * u[0])).astype(np.float32) for u in uniform]

    real_cuda, real_rand, real_conv1d = torch.Tensor.cuda, np.random.rand, torch.nn.functional.conv1d
    torch.Tensor.cuda = lambda self, *a, **k: self
    kept = []

    def conv1d_keep(*a, **k):
        kept.append(real_conv1d(*a, **k))
        return kept[-1]

    try:
        stft = ref_stft.TacotronSTFT(1024, 256, 1024, 80, G.SR, G.FMIN, G.FMAX)
        fn = stft.stft_fn
        basis = fn.forward_basis.numpy().reshape(1026, 1024)
        inv = fn.inverse_basis.numpy().reshape(1026, 1024)
        ref_inverse, ref_gl, specs = [], [], []
        for b, t in enumerate(frames):
            m, a = torch.from_numpy(mags[b])[None], torch.from_numpy(angles[b])[None]
            out = fn.inverse(m, a)
            assert out.shape == (1, 1, 256 * (t - 1))
            ref_inverse.append(out[0, 0].numpy().copy())
            if t >= 4:
                np.random.rand = lambda *shape, _u=uniform[b]: _u.reshape(shape)
                sig = ref_ap.griffin_lim(m, fn, AI.GL_ITERS)
                np.random.rand = real_rand
                assert sig.shape == (1, 256 * (t - 1))
                ref_gl.append(sig[0].numpy().copy())
            else:
                try:
                    ref_ap.griffin_lim(m, fn, 1)
                    raise AssertionError("the reference's griffin_lim ran on 3 frames")
                except RuntimeError:
                    pass  # reflect padding of 512 needs more than 512 samples
            torch.nn.functional.conv1d = conv1d_keep
            _, phase = fn.transform(torch.from_numpy(z["wavs"][b])[None])
            torch.nn.functional.conv1d = real_conv1d
            specs.append(kept.pop()[0].numpy().copy())
            if b == 2:
                phase_u2 = phase[0].numpy().copy()
        assert fn.inverse(torch.ones(1, 513, 1), torch.zeros(1, 513, 1)).shape == (1, 1, 0)
        wsums = {t: ref_ap.window_sumsquare("hann", t, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
                 for t in AI.WSUM_T}

        got = {}
        stft._stft_fn = fn
        ref_tools.griffin_lim = lambda magnitudes, stft_fn, n_iters: (
            got.update(mag=magnitudes.numpy().copy()), torch.zeros(1, 256 * (magnitudes.shape[-1] - 1)))[1]
        ref_tools.write = lambda path, sr, audio: None
        with tempfile.TemporaryDirectory() as tmp:
            ref_tools.inv_mel_spec(torch.from_numpy(np.ascontiguousarray(z["ref_mel_list"][3].T)),
                                   os.path.join(tmp, "a.wav"), stft, 2)
        spec_from_mel = got["mag"][0]
        assert spec_from_mel.shape == (513, frames[3] - 1)
    finally:
        torch.Tensor.cuda, np.random.rand, torch.nn.functional.conv1d = real_cuda, real_rand, real_conv1d

    for t, w in wsums.items():
        assert np.array_equal(w, window_sumsquare("hann", t)), t
        if t >= 2:
            kept_part = w[512:len(w) - 512]
            print(f"window sum over the kept samples, T = {t}: min {kept_part.min():.4f}")
            assert kept_part.min() >= 1.25

    # the reference's own distance from the float64 restatement
    W_inv = W_edge = W_gl = Z = 0.0
    for b, t in enumerate(frames):
        ws = wsums[t] if t in wsums else window_sumsquare("hann", t)
        w64 = AI.istft64(AI.recombine64(mags[b], angles[b]), inv, ws)
        W_inv, W_edge = max(W_inv, AI.stat_W(ref_inverse[b], w64)), max(W_edge, AI.stat_W_edge(ref_inverse[b], w64))
        Z = max(Z, AI.stat_Z(specs[b], AI.transform64(z["wavs"][b], basis)))
        if t >= 4:
            g64 = AI.gl64(mags[b], angles[b], AI.GL_ITERS, basis, inv, ws)
            W_gl = max(W_gl, AI.stat_W(ref_gl[b - 1], g64))
    ref_stats = np.array([W_inv, W_edge, W_gl, Z])
    print("reference f32 vs float64 restatement: W_inv %.3e  W_inv_edge %.3e  W_gl(%d) %.3e  Z %.3e"
          % (W_inv, W_edge, AI.GL_ITERS, W_gl, Z))

    rows = np.array([0, 1, 37, 255, 512, 513, 514, 700, 1025])
    n = save_npz_parts(
        os.path.join(HERE, "audio_inv_a.npz"), angles=np.concatenate([a.reshape(-1) for a in angles]),
        ref_inverse=np.concatenate(ref_inverse), ref_gl=np.concatenate(ref_gl), inv_row_ids=rows, inv_rows=inv[rows],
        phase_u2=phase_u2, spec_from_mel=spec_from_mel, ref_stats=ref_stats,
        **{f"wsum_{t}": w for t, w in wsums.items()})
    print("wrote audio_inv_a.npz in", n, "part(s)")


if __name__ == "__main__":
    main()
