#!/usr/bin/env python3
"""Time fs2_phase_vocoder (include/fs2hip_pvoc.h) on a corpus-like batch, and the same stretch composed of
torch operations in float64 on the same GPU.

    python tools/pvoc_probe.py [--reps 50] [--rounds 5] [--out profiles/pvoc/headline_runs.txt]

64 utterances of 860 frames (10 s at 22,050 Hz, hop 256), 513 bins, rates spread over [0.8, 1.25], on device
buffers allocated once. Each round is event-timed over --reps calls after a warm-up: the C entry point
itself through ctypes, so that no torch operation of the wrapper is inside the window. One JSON line per
round and mode; the lines are also appended to --out.

Bytes. The launch has to read every input frame once and write every output frame: 8 * NB * (T + J) bytes
per row (f32, two parts); that over the elapsed time is given as a fraction of 8.0 TB/s (the HBM3E
data-sheet peak; a float4 copy reaches about 6.3 TB/s on this part). J_max columns are written per row,
the zero tail included; the figure counts the live ones only.

The yardstick is librosa's rule in torch on the same device, float64: magnitudes and angles of the two
gathered frames, the wrapped phase advance, a cumsum over time, torch.polar, the cast. It is the angle
form, so it is close to the kernel's result (the largest difference relative to the row's largest
magnitude is printed), not equal to it.
"""
import argparse
import ctypes
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def torch_stretch(spec, rates, J, hop=256):
    """The angle form over a batch whose rows all have T frames: recomb f32 [B, 2 NB, J_max]."""
    B, nb2, T = spec.shape
    NB = nb2 // 2
    J_max = int(J.max())
    D = torch.complex(spec[:, :NB].double(), spec[:, NB:].double())
    D = torch.nn.functional.pad(D, (0, 2))
    j = torch.arange(J_max, device=spec.device, dtype=torch.float64)
    p = j[None, :] * rates[:, None]
    live = j[None, :] < J[:, None]
    p = torch.where(live, p, torch.zeros_like(p))
    i = p.floor().long()
    alpha = (p - i)[:, None, :]
    idx = i[:, None, :].expand(B, NB, J_max)
    c0, c1 = torch.gather(D, 2, idx), torch.gather(D, 2, idx + 1)
    mag = (1.0 - alpha) * c0.abs() + alpha * c1.abs()
    phi = torch.linspace(0.0, math.pi * hop, NB, device=spec.device, dtype=torch.float64)[None, :, None]
    dphase = c1.angle() - c0.angle() - phi
    dphase = dphase - 2.0 * math.pi * torch.round(dphase / (2.0 * math.pi))
    step = phi + dphase
    acc = D[:, :, :1].angle() + torch.cumsum(step, dim=2) - step  # exclusive: frame j has the steps below j
    out = torch.polar(mag, acc) * live[:, None, :]
    return torch.cat([out.real, out.imag], dim=1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pvoc", "headline_runs.txt"))
    a = ap.parse_args()
    from fs2amd import _lib as L_, ops

    lib = L_.load()
    dev = torch.device("cuda:0")
    B, NB, T = 64, 513, 860
    g = torch.Generator(device="cpu").manual_seed(5)
    # partials that rotate steadily, with noise: neighbouring frames are correlated as an STFT's are
    t = torch.arange(T, dtype=torch.float64)[None, None, :]
    w = (torch.rand(B, NB, 1, generator=g, dtype=torch.float64) - 0.5) * 6.0
    amp = (0.2 + torch.rand(B, NB, 1, generator=g, dtype=torch.float64)).expand(B, NB, T).contiguous()
    z = torch.polar(amp, w * t) \
        + 0.1 * torch.complex(torch.randn(B, NB, T, generator=g, dtype=torch.float64),
                              torch.randn(B, NB, T, generator=g, dtype=torch.float64))
    spec = torch.cat([z.real, z.imag], dim=1).float().to(dev)
    rates_h = np.linspace(0.8, 1.25, B)
    J_h = np.array([ops.pvoc_frames(T, r) for r in rates_h], dtype=np.int64)
    J_max = int(J_h.max())
    rates = torch.from_numpy(rates_h).to(dev)
    frames = torch.full((B,), T, dtype=torch.int64, device=dev)
    J = torch.from_numpy(J_h).to(dev)
    recomb = torch.empty(B, 2 * NB, J_max, device=dev, dtype=torch.float32)
    frames_out = torch.empty(B, device=dev, dtype=torch.int64)
    stream = ops._stream(spec)
    d = L_.PvocDesc()
    d.spec, d.spec_row_stride, d.frames, d.rates = spec.data_ptr(), T, frames.data_ptr(), rates.data_ptr()
    d.B, d.NB, d.T_max, d.J_max = B, NB, T, J_max
    d.recomb, d.recomb_row_stride, d.frames_out = recomb.data_ptr(), J_max, frames_out.data_ptr()

    def kernel():
        L_.check(lib.fs2_phase_vocoder(ctypes.byref(d), stream), "fs2_phase_vocoder")

    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        for rnd in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            yield rnd, e0.elapsed_time(e1) / a.reps

    shape = {"utterances": B, "bins": NB, "frames": T, "rates": [0.8, 1.25], "J_max": J_max, "reps": a.reps}
    nbytes = int(8 * NB * (B * T + J_h.sum()))
    for rnd, ms in timed(kernel):
        emit(dict(shape, mode="fs2_phase_vocoder", round=rnd, ms_per_call=round(ms, 4), bytes=nbytes,
                  gbytes_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1),
                  fraction_of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)))
    for rnd, ms in timed(lambda: torch_stretch(spec, rates, J)):
        emit(dict(shape, mode="torch composition float64 (abs, angle, cumsum, polar)", round=rnd,
                  ms_per_call=round(ms, 4)))
    ref = torch_stretch(spec, rates, J)
    kernel()
    torch.cuda.synchronize(dev)
    scale = spec.abs().amax(dim=(1, 2), keepdim=True)
    emit({"check": "the angle form in torch against the kernel's rotor form, relative to the row's largest input value",
          "frames_out_equal": bool((frames_out == J).all()),
          "max_relative_difference": float(((ref - recomb).abs() / scale).max())})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
