#!/usr/bin/env python3
"""Generate the mixture / curve conditioning fixtures (condmix_a.npz, condmix_b.npz) by running the
REFERENCE itself: eval mode, fp32, CPU, weights from fs2amd.synth_weights seed 0, free-running (as
gen_golden_prosody.py; gen_golden.py's import_reference / t2n / save_npz_parts are reused by import).

The reference's forward() looks its four conditioning ids up in nn.Embedding tables
(model/fastspeech2.py:101-110). forward_mix() below drives the reference's OWN sub-modules in
forward()'s order (model/fastspeech2.py:92-148: masks, encoder, speaker add, emotion Linear + ReLU
add, variance adaptor, decoder, mel_linear, postnet) with ``weights @ embedding.weight`` in place of
each lookup. main() first asserts that this sequence, run with one-hot weights, reproduces
``model(**args)`` with the ids EXACTLY (all ten outputs), then runs it with the weights below.

    fixture     batch                                           weight seed  forms
    condmix_a   synth_batch(3, 5, 17, seed=100, teacher=False)      58         [B, n] mixtures on all four inputs
    condmix_b   synth_batch(3, 5, 17, seed=101, teacher=False)      116        emotions a curve [B, L, n] (three
                                                                             keyframes per utterance), arousals a
                                                                             mixture [B, n], valences and speakers ids

Weights (rows(), per input / keyframe set): random positive rows normalised to sum 1 on the host;
utterance 1's rows are then scaled to sum 1.4 (intensity), utterance 2's first entry is negated
(extrapolation). Nothing is normalised after that: the model uses weights as given.

The seeds were chosen (search(): the first weight seed that passes) so that the reference sits
clear of every discrete decision, with the margins gen_golden_prosody.py asserts: every pitch /
energy prediction at a valid position at least 1e-3 from the nearest bin edge, every exp(log_d) - 1
at least 6e-3 from a .5 rounding tie. main() asserts them, prints them and stores them
(``margins`` = pitch, energy, tie).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_condmix.py [search]
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
from gen_golden_prosody import EDGE_MARGIN, TIE_MARGIN, margins  # noqa: E402

# fixture -> (batch seed, weight seed, curves?)
CASES = {"condmix_a": (100, 58, False), "condmix_b": (101, 116, True)}
NAMES = ("speakers", "emotions", "arousals", "valences")


def rows(g, B, n):
    """[B, n]: positive rows of sum 1; row 1 scaled to sum 1.4; row 2 with its first entry negated."""
    w = 0.05 + torch.rand(B, n, generator=g)
    w = w / w.sum(1, keepdim=True)
    w[1] *= 1.4
    w[2, 0] = -w[2, 0]
    return w


def make_weights(model, args, seed, curves):
    from fs2amd.emotion import curve

    g = torch.Generator().manual_seed(seed)
    B, L = args["texts"].shape
    n = {"speakers": model.speaker_emb.num_embeddings, "emotions": model.emotion_emb.num_embeddings,
         "arousals": model.arousal_emb.num_embeddings, "valences": model.valence_emb.num_embeddings}
    if not curves:
        return {k: rows(g, B, n[k]) for k in NAMES}
    keys = [rows(g, B, n["emotions"]) for _ in range(3)]  # the rows at phoneme 0, the middle, the last one
    emo = torch.stack([curve([(0, keys[0][b]), (int(args["src_lens"][b]) // 2, keys[1][b]),
                              (int(args["src_lens"][b]) - 1, keys[2][b])], int(args["src_lens"][b]), L)
                       for b in range(B)])
    return {"speakers": args["speakers"], "emotions": emo, "arousals": rows(g, B, n["arousals"]),
            "valences": args["valences"]}


def as_weights(t, n):
    return torch.nn.functional.one_hot(t, n).float() if not t.is_floating_point() else t


def forward_mix(model, args, w):
    """The reference's forward() (model/fastspeech2.py:92-148) through its own sub-modules, free-running,
    controls 1.0, with w[name] @ embedding.weight in place of embedding(ids)."""
    from utils.tools import get_mask_from_lengths

    texts, src_lens, L = args["texts"], args["src_lens"], args["max_src_len"]
    tab = {"speakers": model.speaker_emb.weight, "emotions": model.emotion_emb.weight,
           "arousals": model.arousal_emb.weight, "valences": model.valence_emb.weight}
    w = {k: as_weights(w[k], tab[k].shape[0]) for k in NAMES}
    src_masks = get_mask_from_lengths(src_lens, L)                               # :92
    output = model.encoder(texts, src_masks)                                     # :99
    output = output + (w["speakers"] @ tab["speakers"]).unsqueeze(1).expand(-1, L, -1)   # :101-104
    if any(w[k].dim() == 3 for k in NAMES[1:]):  # a curve: the other two broadcast over L
        w = {k: (v if v.dim() == 3 or k == "speakers" else v.unsqueeze(1).expand(-1, L, -1)) for k, v in w.items()}
    emb = torch.cat([w[k] @ tab[k] for k in NAMES[1:]], dim=-1)                  # :107
    emo = model.emotion_linear(emb)
    output = output + (emo if emo.dim() == 3 else emo.unsqueeze(1).expand(-1, L, -1))    # :108-110
    (output, p_pred, e_pred, log_d, d_rounded, mel_lens, mel_masks) = model.variance_adaptor(   # :112-131
        output, src_masks, None, None, None, None, None, 1.0, 1.0, 1.0)
    output, mel_masks = model.decoder(output, mel_masks)                         # :133
    output = model.mel_linear(output)                                            # :134
    postnet_output = model.postnet(output) + output                              # :136
    return (output, postnet_output, p_pred, e_pred, log_d, d_rounded, src_masks, mel_masks, src_lens, mel_lens)


def run(model, args, seed, curves):
    w = make_weights(model, args, seed, curves)
    with torch.no_grad():
        outs = forward_mix(model, args, w)
    va = model.variance_adaptor
    m = margins(t2n(outs[2]), t2n(outs[3]), t2n(outs[4]), t2n(outs[6]), t2n(va.pitch_bins), t2n(va.energy_bins))
    return w, outs, m


def build_model():
    FastSpeech2, LR = import_reference()
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="fs2_golden_")
    C.write_side_files(tmp)
    pc, mc, _ = C.synthetic_configs(tmp)
    model = FastSpeech2(pc, mc)
    fill_module(model, seed=0)
    model.eval()
    torch.set_num_threads(8)
    return model, LR


def search(n_seeds=200):
    model, _ = build_model()
    for name, (seed, _, curves) in CASES.items():
        args = synth_batch(3, 5, 17, seed=seed, teacher=False)
        for ws in range(n_seeds):
            m = run(model, args, ws, curves)[2]
            if m[0] >= EDGE_MARGIN and m[1] >= EDGE_MARGIN and m[2] >= TIE_MARGIN:
                print(f"{name}: weight seed {ws} margins pitch {m[0]:.3e} energy {m[1]:.3e} tie {m[2]:.4f}")
                break
        else:
            print(f"{name}: no seed below {n_seeds}")


def main():
    model, LR = build_model()
    for name, (seed, wseed, curves) in CASES.items():
        args = synth_batch(3, 5, 17, seed=seed, teacher=False)
        # the sequence itself: one-hot weights reproduce the reference's forward with the ids exactly
        with torch.no_grad():
            ref = model(**args)
            hot = forward_mix(model, args, {k: args[k] for k in NAMES})
        for k, a, b in zip(OUT_NAMES, ref, hot):
            assert a.shape == b.shape and torch.equal(a, b), (name, k)
        w, outs, m = run(model, args, wseed, curves)
        rec = {"in_" + k: t2n(v) for k, v in args.items() if v is not None}
        for k in NAMES:
            rec["w_" + k] = t2n(w[k])
        rec["controls"] = np.array([1.0, 1.0, 1.0])
        for k, v in zip(OUT_NAMES, outs):
            rec["out_" + k] = t2n(v)
        rec["lr_index_map"], rec["lr_mel_len"] = index_map(LR, outs[5], None)
        rec["margins"] = np.array(m, dtype=np.float64)
        rec["pitch_bins"], rec["energy_bins"] = t2n(model.variance_adaptor.pitch_bins), t2n(
            model.variance_adaptor.energy_bins)
        print(f"{name}: src_lens {rec['in_src_lens'].tolist()} mel_lens {rec['out_mel_lens_out'].tolist()} margins "
              f"pitch {m[0]:.3e} energy {m[1]:.3e} tie {m[2]:.4f}; weight sums "
              f"{ {k: np.round(np.asarray(rec['w_' + k], np.float64).sum(-1).reshape(-1)[:3], 3).tolist() for k in NAMES if rec['w_' + k].dtype.kind == 'f'} }")
        assert m[0] >= EDGE_MARGIN and m[1] >= EDGE_MARGIN and m[2] >= TIE_MARGIN, (name, m)
        path = os.path.join(HERE, name + ".npz")
        save_npz_parts(path, **rec)
        print(f"{name}: {os.path.getsize(path) / 1e3:.1f} kB  mel {tuple(outs[0].shape)}")


if __name__ == "__main__":
    search() if sys.argv[1:2] == ["search"] else main()
