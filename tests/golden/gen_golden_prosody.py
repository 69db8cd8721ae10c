#!/usr/bin/env python3
"""Generate the per-phoneme control-map fixtures (prosody_a.npz, prosody_b.npz) by running the
REFERENCE itself: eval mode, fp32, CPU, weights from fs2amd.synth_weights seed 0 (as gen_golden.py,
whose import_reference / t2n / save_npz_parts are reused by import).

The reference's VarianceAdaptor multiplies the pitch / energy predictions and the rounded
durations by ``control`` (model/modules.py:80-100,117-135): a plain broadcast, so a [B, L_src]
tensor gives every phoneme its own factor. Each fixture stores the inputs, both maps
(``map_p_control``, ``map_d_control``; e_control = 1.0), the ten outputs and the LR index map.

    fixture     batch                                          map seed  src_lens      mel_lens
    prosody_a   synth_batch(3, 5, 17, seed=100, teacher=False)   20      [13, 13, 7]   [70, 145, 67]
    prosody_b   synth_batch(3, 5, 17, seed=101, teacher=False)   18      [17, 14, 12]  [34, 18, 42]

Maps: g = torch.Generator().manual_seed(s); p_control = 0.5 + 1.5 * rand(B, L, generator=g), then
d_control the same way from the same generator.

The seeds were chosen so that the reference sits clear of every discrete decision (the project's
fp32 prediction tolerance is 5e-4, times a control of at most 2): every scaled pitch / energy
prediction at a valid position is at least 1e-3 from the nearest bin edge and every exp(log_d) - 1
at least 6e-3 from a .5 rounding tie. main() asserts those conditions and prints the margins found
(pitch / energy / tie): a 1.17e-3 / 1.55e-3 / 0.028, b 1.30e-3 / 1.18e-3 / 0.0106.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_prosody.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import (OUT_NAMES, C, fill_module, import_reference, index_map, save_npz_parts,  # noqa: E402
                        synth_batch, t2n)

CASES = {"prosody_a": (100, 20), "prosody_b": (101, 18)}
EDGE_MARGIN, TIE_MARGIN = 1e-3, 6e-3


def control_maps(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    p = 0.5 + 1.5 * torch.rand(B, L, generator=g)
    d = 0.5 + 1.5 * torch.rand(B, L, generator=g)
    return p, d


def margins(p_pred, e_pred, log_d, src_masks, pitch_bins, energy_bins):
    """(pitch, energy, tie): the smallest distance of a scaled prediction at a valid position to a
    bin edge, and of exp(log_d) - 1 at a valid position to a .5 rounding tie (float64 on the stored
    f32 values)."""
    valid = ~np.asarray(src_masks, dtype=bool)
    edge = lambda v, bins: float(np.abs(np.asarray(v, np.float64)[valid][:, None] -
                                        np.asarray(bins, np.float64)[None, :]).min())
    d = np.exp(np.asarray(log_d, np.float32))[valid].astype(np.float64) - 1.0
    tie = float(np.abs(d - np.floor(d) - 0.5).min())
    return edge(p_pred, pitch_bins), edge(e_pred, energy_bins), tie


def main():
    FastSpeech2, LR = import_reference()
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="fs2_golden_")
    C.write_side_files(tmp)
    pc, mc, _ = C.synthetic_configs(tmp)
    model = FastSpeech2(pc, mc)
    fill_module(model, seed=0)
    model.eval()
    torch.set_num_threads(8)
    va = model.variance_adaptor
    for name, (seed, map_seed) in CASES.items():
        args = synth_batch(3, 5, 17, seed=seed, teacher=False)
        B, L = args["texts"].shape
        p_map, d_map = control_maps(B, L, map_seed)
        with torch.no_grad():
            outs = model(**args, p_control=p_map, e_control=1.0, d_control=d_map)
        rec = {"in_" + k: t2n(v) for k, v in args.items() if v is not None}
        rec["map_p_control"], rec["map_d_control"] = t2n(p_map), t2n(d_map)
        rec["controls"] = np.array([np.nan, 1.0, np.nan])  # p and d are the maps above
        for k, v in zip(OUT_NAMES, outs):
            rec["out_" + k] = t2n(v)
        rec["lr_index_map"], rec["lr_mel_len"] = index_map(LR, outs[5], None)
        m = margins(rec["out_p_pred"], rec["out_e_pred"], rec["out_log_d"], rec["out_src_masks"],
                    t2n(va.pitch_bins), t2n(va.energy_bins))
        valid = ~rec["out_src_masks"]
        dr = rec["out_d_rounded"][valid]
        print(f"{name}: src_lens {rec['in_src_lens'].tolist()} mel_lens {rec['out_mel_lens_out'].tolist()} margins "
              f"pitch {m[0]:.3e} energy {m[1]:.3e} tie {m[2]:.4f}; zero-frame phonemes "
              f"{int((np.trunc(dr) == 0).sum())}, fractional d_rounded {int((dr != np.trunc(dr)).sum())}")
        assert m[0] >= EDGE_MARGIN and m[1] >= EDGE_MARGIN and m[2] >= TIE_MARGIN, (name, m)
        path = os.path.join(HERE, name + ".npz")
        save_npz_parts(path, **rec)
        print(f"{name}: {os.path.getsize(path) / 1e3:.1f} kB  mel {tuple(outs[0].shape)}")


if __name__ == "__main__":
    main()
