#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the REFERENCE itself.

Runs only in the build container, where the reference tree is mounted read-only at
/root/reference (it never travels to the GPU box; only the .npz/.json outputs do).

* Imports the reference's ``model.FastSpeech2`` / ``model.modules.LengthRegulator`` with six
  text-frontend modules stubbed (unidecode, inflect, quickspacer, g2pk, jamo, jamo.jamo:
  ordinary ModuleNotFoundErrors) and synthetic side files
  (stats/speakers/emotions.json) in a temp ``preprocessed_path``.
* Fills the 240-key state_dict from the counter-based generator
  ``fs2amd.synth_weights`` (seed 0), runs eval-mode fp32 forwards on CPU and writes
  inputs + the 10-tuple outputs (+ LR source-index maps captured through the reference's
  own LengthRegulator on an index-valued input).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FS2_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd"))
sys.path.insert(0, os.path.dirname(HERE))

from fs2amd import config as C  # noqa: E402
from fs2amd.data import synth_batch  # noqa: E402
from fs2amd.synth_weights import fill_module  # noqa: E402

from _npz_parts import save_npz_parts  # noqa: E402  (no file under tests/golden/ above 1 MiB)


def _stub(name):
    mod = types.ModuleType(name)

    def ga(attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        return lambda *a, **k: None

    mod.__getattr__ = ga
    mod.__path__ = []
    return mod


def import_reference():
    for m in ["unidecode", "inflect", "quickspacer", "g2pk", "jamo", "jamo.jamo"]:
        sys.modules.setdefault(m, _stub(m))
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from model import FastSpeech2  # noqa
    from model.modules import LengthRegulator  # noqa
    return FastSpeech2, LengthRegulator


def t2n(v):
    if v is None:
        return None
    if torch.is_tensor(v):
        return v.detach().cpu().numpy()
    return np.asarray(v)


OUT_NAMES = ["mel", "postnet_mel", "p_pred", "e_pred", "log_d", "d_rounded", "src_masks", "mel_masks",
             "src_lens_out", "mel_lens_out"]


def index_map(LR, duration, max_len):
    """Reference LengthRegulator applied to x[b,i,0] = i+1 -> source index per frame (-1 = pad)."""
    B, L = duration.shape
    idx = (torch.arange(L, dtype=torch.float64) + 1).view(1, L, 1).expand(B, L, 1).contiguous()
    out, mel_len = LR()(idx, duration, max_len)
    return (out[..., 0].round().to(torch.int64) - 1).numpy().astype(np.int32), mel_len.numpy()


def run_case(model, LR, name, args, controls=(1.0, 1.0, 1.0), save_full=True, head=0, frames=()):
    p_c, e_c, d_c = controls
    with torch.no_grad():
        outs = model(**args, p_control=p_c, e_control=e_c, d_control=d_c)
    rec = {}
    for k, v in args.items():
        if v is None:
            continue
        rec["in_" + k] = t2n(v)
    rec["controls"] = np.array(controls, dtype=np.float64)
    for k, v in zip(OUT_NAMES, outs):
        if save_full:
            rec["out_" + k] = t2n(v)
    dur = outs[5] if args.get("d_targets") is None else args["d_targets"]
    max_len = args.get("max_mel_len")
    rec["lr_index_map"], rec["lr_mel_len"] = index_map(LR, dur, max_len)
    if not save_full:
        mel, post = outs[0].double(), outs[1].double()
        mel_lens = outs[9]
        valid = (torch.arange(mel.shape[1])[None, :] < mel_lens[:, None]).double()[..., None]
        rec["ck_mel_valid_sum"] = (mel * valid).sum((1, 2)).numpy()
        rec["ck_post_valid_sum"] = (post * valid).sum((1, 2)).numpy()
        rec["ck_post_valid_abs"] = (post.abs() * valid).sum((1, 2)).numpy()
        rec["ck_post_all_sum"] = post.sum((1, 2)).numpy()
        rec["ck_post_sq"] = (post * post).sum((1, 2)).numpy()
        for k in ("p_pred", "e_pred", "log_d", "d_rounded", "mel_lens_out", "src_masks", "mel_masks"):
            rec["out_" + k] = t2n(outs[OUT_NAMES.index(k)])
        rec["out_shape_mel"] = np.array(outs[0].shape)
    if head:  # the full outputs of the first `head` utterances
        rec["out_mel_head"] = t2n(outs[0][:head])
        rec["out_postnet_mel_head"] = t2n(outs[1][:head])
    for a, b in frames:  # frame slices of every utterance
        rec[f"out_postnet_mel_f{a}_{b}"] = t2n(outs[1][:, a:b])
    path = os.path.join(HERE, name + ".npz")
    save_npz_parts(path, **rec)
    print(f"{name}: {os.path.getsize(path) / 1e3:.1f} kB  mel {tuple(outs[0].shape)}")


def lr_cases(LR):
    g = torch.Generator().manual_seed(7)
    cases = {}
    x = torch.randn(3, 7, 5, generator=g)
    cases["int"] = (x, torch.tensor([[2, 0, 3, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1], [0, 4, 0, 0, 2, 0, 0]]), None)
    cases["float_trunc"] = (x, torch.tensor([[2.7, 0.4, -1.5, 3.0, 1.999, 0.0, 0.0],
                                             [1.0, -0.0, 5.5, 0.0, 0.0, 0.0, 0.0],
                                             [0.9, 0.9, 0.9, 0.9, 2.01, 0.0, 1.0]]), None)
    cases["pad_longer"] = (x, cases["int"][1], 12)
    cases["crop_shorter"] = (x, cases["int"][1], 4)
    cases["zero_row"] = (x, torch.tensor([[0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 2], [1, 2, 3, 0, 0, 0, 0]]), None)
    cases["nonzero_padding_slots"] = (x, torch.tensor([[1, 1, 1, 9, 9, 0, 0], [2, 2, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0, 7]]), 30)
    rec = {}
    for name, (xx, d, max_len) in cases.items():
        out, mel_len = LR()(xx, d, max_len)
        rec[f"{name}__x"] = xx.numpy()
        rec[f"{name}__d"] = d.numpy()
        rec[f"{name}__max_len"] = np.array(-1 if max_len is None else max_len)
        rec[f"{name}__out"] = out.numpy()
        rec[f"{name}__mel_len"] = mel_len.numpy()
    np.savez_compressed(os.path.join(HERE, "lr_cases.npz"), **rec)
    print("lr_cases:", list(cases))


def train_case(FastSpeech2, pc, mc, sd, name="train_grads", shape=(4, 10, 24), seed=11, d_range=(2, 10)):
    """One reference training step's gradients (train mode: BatchNorm batch statistics, decoder
    crop to max_seq_len), with every dropout disabled so the step is deterministic: nn.Dropout
    modules get p = 0 and the PostNet's hard-coded F.dropout(0.5) (transformer/Layers.py:133-134)
    is replaced by identity for the duration of this case only."""
    import torch.nn.functional as F
    from model.loss import FastSpeech2Loss
    from fs2amd.data import loss_inputs

    m = FastSpeech2(pc, mc)
    m.load_state_dict(sd)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    args = synth_batch(*shape, seed=seed, with_mels=True, pe_targets=True, d_range=d_range)
    orig = F.dropout
    F.dropout = lambda x, p=0.5, training=False, inplace=False: x
    try:
        out = m(**args)
        losses = FastSpeech2Loss(pc, mc)(loss_inputs(args), out)
        losses[0].backward()
    finally:
        F.dropout = orig
    rec = {"in_" + k: t2n(v) for k, v in args.items() if v is not None}
    rec["losses"] = np.array([float(l) for l in losses], dtype=np.float64)
    keys = [k for k, p in m.named_parameters() if p.grad is not None]
    rec["grad_keys"] = np.array(keys)
    rec["grad_sum"] = np.array([float(p.grad.double().sum()) for k, p in m.named_parameters() if k in keys])
    rec["grad_sumsq"] = np.array([float((p.grad.double() ** 2).sum()) for k, p in m.named_parameters() if k in keys])
    g = torch.Generator().manual_seed(3)
    params = dict(m.named_parameters())
    for i, k in enumerate(keys):  # samples keyed by position in grad_keys
        flat = params[k].grad.detach().reshape(-1)
        idx = torch.randint(0, flat.numel(), (16,), generator=g)
        rec[f"gidx_{i}"] = idx.numpy()
        rec[f"gval_{i}"] = flat[idx].numpy()
    for bname, buf in m.named_buffers():
        if "running_" in bname:
            rec["bn_" + bname] = t2n(buf)
    rec["out_mel_lens"] = t2n(out[9])
    path = os.path.join(HERE, name + ".npz")
    save_npz_parts(path, **rec)
    print(f"{name}: {os.path.getsize(path) / 1e3:.1f} kB, {len(keys)} grads, losses {rec['losses']}")


def tiny_model_config(mc):
    """The reference architecture at toy width (checkpoint fixture): 1 encoder / 1 decoder FFT
    block of width 16, FFN 32, VariancePredictor width 16. The PostNet keeps its fixed shape
    (transformer/Layers.py PostNet defaults, 80 -> 512 x 5)."""
    t = dict(mc["transformer"], encoder_layer=1, decoder_layer=1, encoder_hidden=16, decoder_hidden=16,
             conv_filter_size=32)
    return dict(mc, transformer=t, variance_predictor=dict(mc["variance_predictor"], filter_size=16))


def ckpt_case(FastSpeech2, pc, mc):
    """A checkpoint written by the reference's own train loop (train.py:82-97 step, :151-161
    torch.save of {"model", "optimizer"}) after 2 steps of the reference ScheduledOptim
    (model/optimizer.py: non-fused Adam, numpy-float learning rates) at the toy width of
    tiny_model_config; then the reference's step 3: its clipped gradients, the learning rate and
    every parameter after the update. The PostNet is zero and frozen (no gradient, no Adam state:
    its 4.3 M zeros compress away) so the fixture stays small; every other parameter trains.
    Dropout disabled as in train_case."""
    import torch.nn.functional as F
    from model import ScheduledOptim as RefOptim
    from model.loss import FastSpeech2Loss
    from fs2amd.data import loss_inputs

    mct = tiny_model_config(mc)
    tc = C.ESD_TRAIN_CONFIG
    m = FastSpeech2(pc, mct)
    fill_module(m, seed=5)
    for p in m.postnet.parameters():
        p.data.zero_()
        p.requires_grad_(False)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    opt = RefOptim(m, tc, mct, 0)
    loss_fn = FastSpeech2Loss(pc, mct)
    orig = F.dropout
    F.dropout = lambda x, p=0.5, training=False, inplace=False: x

    def step(i, record=False):
        args = synth_batch(2, 8, 12, seed=40 + i, with_mels=True, pe_targets=True)
        out = m(**args)
        losses = loss_fn(loss_inputs(args), out)
        losses[0].backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), tc["optimizer"]["grad_clip_thresh"])
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None} if record else None
        opt.step_and_update_lr()
        opt.zero_grad()
        return grads, losses

    try:
        step(1)
        step(2)
        d = os.path.join(HERE, "ref_ckpt")
        os.makedirs(d, exist_ok=True)
        raw = os.path.join(d, "2.pth.tar")
        torch.save({"model": m.state_dict(), "optimizer": opt._optimizer.state_dict()}, raw)
        # committed gzip-compressed (the zero PostNet is 17 MB of the file); the test restores the
        # exact bytes the reference wrote
        import gzip
        import shutil
        with open(raw, "rb") as fi, gzip.open(raw + ".gz", "wb", compresslevel=9) as fo:
            shutil.copyfileobj(fi, fo)
        os.remove(raw)
        with open(os.path.join(d, "model_config.json"), "w") as f:
            json.dump(mct, f, indent=1, sort_keys=True)
        grads, losses = step(3, record=True)
    finally:
        F.dropout = orig
    keys = sorted(grads)
    params = dict(m.named_parameters())
    rec = {"keys": np.array(keys), "lr": np.array(float(opt._optimizer.param_groups[0]["lr"])),
           "current_step": np.array(opt.current_step), "losses": np.array([float(l.detach()) for l in losses])}
    for i, k in enumerate(keys):
        rec[f"g_{i}"] = t2n(grads[k])
        rec[f"p_{i}"] = t2n(params[k])
    np.savez_compressed(os.path.join(HERE, "ref_ckpt_next.npz"), **rec)
    print(f"ref_ckpt: 2.pth.tar.gz {os.path.getsize(raw + '.gz') / 1e3:.0f} kB, {len(keys)} trained "
          f"params, step-3 lr {rec['lr']}")


def sub_batch(batch, rows, L=None, T=None):
    """Rows of a synth batch, re-padded to L phonemes / T frames (zero / cropped)."""
    out = {}
    for k, v in batch.items():
        out[k] = v[rows] if torch.is_tensor(v) and v.dim() >= 1 else v
    L = int(out["src_lens"].max()) if L is None else L
    out["max_src_len"] = L
    for k in ("texts", "d_targets", "p_targets", "e_targets"):
        if out.get(k) is not None:
            v = out[k]
            out[k] = torch.nn.functional.pad(v, (0, max(0, L - v.shape[1])))[:, :L]
    if out.get("mel_lens") is not None:
        out["mel_lens"] = out["d_targets"].sum(1)
        out["max_mel_len"] = int(out["mel_lens"].max()) if T is None else T
    return out


def padding_class_cases(model, LR):
    """SURVEY.md §8a padding classes, each case a 2-utterance batch whose utterance 0 is the same
    base utterance (20 phonemes, teacher-forced): the output for it depends on the phoneme padding
    L_max - L_0 in {0, 1, >=2} (VariancePredictor receptive field +-2: it reads the conditioning
    vectors and pitch embeddings in padded slots) and on the frame padding T_max - T_0 in
    {0..9, >=10} (PostNet receptive field +-10: it reads mel_linear's bias in padded frames).
    Companions are 1 / 2 / 3 phonemes longer (same frame count as the base), and the same length
    with 9 / 10 / 30 frames more."""
    g = torch.Generator().manual_seed(21)
    base = synth_batch(1, 20, seed=6)
    L0, T0 = 20, int(base["mel_lens"][0])
    for extra in (1, 2, 3):
        comp = synth_batch(1, L0 + extra, seed=30 + extra)
        d = torch.zeros(1, L0 + extra, dtype=torch.int64)
        d[0, :L0 + extra] = 1
        # same total frames as the base: spread T0 frames over L0 + extra phonemes
        q, r = divmod(T0, L0 + extra)
        d[0] = q
        d[0, :r] += 1
        comp["d_targets"], comp["mel_lens"], comp["max_mel_len"] = d, d.sum(1), int(d.sum())
        pair = {k: torch.cat([torch.nn.functional.pad(base[k], (0, extra)) if base[k].dim() == 2 else base[k],
                              comp[k]]) if torch.is_tensor(base[k]) else base[k] for k in base}
        pair["max_src_len"], pair["max_mel_len"] = L0 + extra, max(T0, int(d.sum()))
        run_case(model, LR, f"pad_ph{extra}", pair)
    for extra in (9, 10, 30):
        comp = synth_batch(1, L0, seed=40 + extra)
        d = comp["d_targets"].clone()
        while int(d.sum()) != T0 + extra:  # adjust to exactly T0 + extra frames, durations >= 1
            i = int(torch.randint(0, L0, (1,), generator=g))
            if int(d.sum()) < T0 + extra:
                d[0, i] += 1
            elif d[0, i] > 1:
                d[0, i] -= 1
        comp["d_targets"], comp["mel_lens"], comp["max_mel_len"] = d, d.sum(1), int(d.sum())
        pair = {k: torch.cat([base[k], comp[k]]) if torch.is_tensor(base[k]) else base[k] for k in base}
        pair["max_src_len"], pair["max_mel_len"] = L0, T0 + extra
        run_case(model, LR, f"pad_fr{extra}", pair)


def vocoder_case():
    """The reference HiFi-GAN generator (hifigan/models.py, V1 config.json) with counter-generated
    weights (fs2amd.synth_weights.fill_vocoder, seed 0), eval, fp32 CPU, on two mel batches: the
    reference FastSpeech2's own postnet output of cfg1_teacher ([1, 207, 80]) and of the first two
    mini_teacher utterances (padded batch). Stores inputs [B, 80, T] and wavs [B, 1, T*256]; also
    the generator's state_dict key list (drop-in key compatibility)."""
    sys.path.insert(0, REF)
    import hifigan
    from fs2amd.synth_weights import fill_vocoder

    with open(os.path.join(REF, "hifigan", "config.json")) as f:
        h = json.load(f)
    g = hifigan.Generator(hifigan.AttrDict(h))
    fill_vocoder(g, h, seed=0)
    g.eval()
    rec = {"keys": np.array(list(g.state_dict().keys()))}
    c1 = np.load(os.path.join(HERE, "cfg1_teacher.npz"))["out_postnet_mel"]
    mt = np.load(os.path.join(HERE, "mini_teacher.npz"))["out_postnet_mel"][:2]
    for name, mel in (("cfg1", c1), ("mini2", mt)):
        x = torch.from_numpy(mel).transpose(1, 2).contiguous()
        with torch.no_grad():
            y = g(x)
        rec[f"{name}__mel"] = x.numpy()
        rec[f"{name}__wav"] = y.numpy()
        print(f"vocoder {name}: mel {tuple(x.shape)} -> wav {tuple(y.shape)}, |wav| max {float(y.abs().max()):.3f} "
              f"std {float(y.std()):.3f}")
    np.savez_compressed(os.path.join(HERE, "vocoder.npz"), **rec)


def pipeline_case(pc, mc):
    """The reference's own batch assembly (dataset_chinese.py Dataset / TextDataset collate_fn and
    utils/tools.py to_device on CPU) over the deterministic synthetic corpus
    fs2amd.pipeline.write_synthetic_corpus(dir, 24, seed=0, long_every=11): every array of every
    15- / 9-tuple (batch_size 4, sorted and unsorted, drop_last both ways)."""
    from fs2amd.pipeline import write_synthetic_corpus
    from fs2amd import config as C
    sys.path.insert(0, REF)
    import dataset_chinese as D
    from utils.tools import to_device

    d = write_synthetic_corpus(tempfile.mkdtemp(prefix="fs2_corpus_"), 24, seed=0, long_every=11, max_seq_len=2000)
    pc = dict(pc, path={"preprocessed_path": d})
    tc = C.ESD_TRAIN_CONFIG
    rec = {}
    for tag, (fname, sort, drop) in {"train_sorted": ("train.txt", True, False), "train_drop": ("train.txt", True, True),
                                      "val_plain": ("val.txt", False, False)}.items():
        ds = D.Dataset(fname, pc, mc, tc, sort=sort, drop_last=drop)
        batches = ds.collate_fn([ds[i] for i in range(len(ds))])
        rec[f"{tag}__n"] = np.array(len(batches))
        for j, b in enumerate(batches):
            tb = to_device(b, torch.device("cpu"))
            for k, v in enumerate(tb):
                key = f"{tag}__{j}__{k}"
                if torch.is_tensor(v):
                    rec[key] = v.numpy()
                    rec[key + "__dtype"] = np.array(str(v.dtype))
                elif isinstance(v, list):
                    rec[key] = np.array(v)
                else:
                    rec[key] = np.array(v)
    td = D.TextDataset(os.path.join(d, "val.txt"), pc, mc)
    tb = to_device(td.collate_fn([td[i] for i in range(len(td))]), torch.device("cpu"))
    for k, v in enumerate(tb):
        rec[f"text__{k}"] = v.numpy() if torch.is_tensor(v) else np.array(v)
        if torch.is_tensor(v):
            rec[f"text__{k}__dtype"] = np.array(str(v.dtype))
    save_npz_parts(os.path.join(HERE, "pipeline_batches.npz"), **rec)
    print("pipeline_batches:", {k: int(v) for k, v in rec.items() if k.endswith("__n")})


def main(only=None, only2=None):
    FastSpeech2, LR = import_reference()
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="fs2_golden_")
    C.write_side_files(tmp)
    pc, mc, _ = C.synthetic_configs(tmp)
    model = FastSpeech2(pc, mc)
    fill_module(model, seed=0)
    model.eval()
    torch.set_num_threads(8)

    sd = model.state_dict()
    if only == "train":
        train_case(FastSpeech2, pc, mc, sd)
        return
    if only == "pipeline":
        pipeline_case(pc, mc)
        return
    if only == "vocoder":
        vocoder_case()
        return
    if only == "round3":  # round-3 additions (earlier fixtures stay byte-identical)
        if only2 in (None, "targets"):
            # teacher-forced durations AND pitch / energy targets at the bench shapes: no bucket of
            # the bf16 path can flip, so bf16 is checked against the reference at full size
            run_case(model, LR, "cfg2_targets", synth_batch(64, 64, seed=1, pe_targets=True), save_full=False, head=4)
            run_case(model, LR, "cfg4_targets", synth_batch(256, 16, 160, seed=1, pe_targets=True), save_full=False,
                     head=2)
        if only2 in (None, "long"):
            # eval with 2004 phonemes / 2004 frames > max_seq_len 2000: both PE recompute branches
            # (transformer/Models.py:82-87 encoder, :145-152 decoder)
            run_case(model, LR, "long_eval", synth_batch(1, 2004, seed=8, d_range=(1, 1), pe_targets=True),
                     save_full=False, frames=((0, 32), (1960, 2004)))
        if only2 in (None, "crop"):
            # train mode with mel lengths > max_seq_len: the decoder crops to 2000 frames
            # (Models.py:154-162) and FastSpeech2Loss crops the targets to the mask (loss.py:33-36)
            train_case(FastSpeech2, pc, mc, sd, name="train_crop", shape=(2, 200, 230), seed=13, d_range=(9, 10))
        if only2 in (None, "ckpt"):
            ckpt_case(FastSpeech2, pc, mc)
        return
    if only == "round2":  # round-2 additions (the round-1 fixtures above stay byte-identical)
        if only2 != "train16":
            padding_class_cases(model, LR)
            run_case(model, LR, "cfg2_free", synth_batch(64, 64, seed=1, teacher=False), save_full=False)
        train_case(FastSpeech2, pc, mc, sd, name="train_b16", shape=(16, 16, 64), seed=12)
        return
    manifest = {"reference": REF, "torch": torch.__version__, "weights_seed": 0, "n_keys": len(sd), "keys": {}}
    for k, v in sd.items():
        a = v.detach().double()
        manifest["keys"][k] = {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", ""),
                               "sum": float(a.sum()), "sumsq": float((a * a).sum()),
                               "sha256": hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}
    with open(os.path.join(HERE, "weights_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
    print("manifest:", len(sd), "keys")

    lr_cases(LR)
    run_case(model, LR, "cfg1_teacher", synth_batch(1, 32, seed=1))
    run_case(model, LR, "cfg1_free", synth_batch(1, 32, seed=1, teacher=False))
    run_case(model, LR, "mini_teacher", synth_batch(4, 12, 40, seed=2))
    run_case(model, LR, "mini_targets", synth_batch(4, 10, 36, seed=3, pe_targets=True), controls=(0.8, 1.2, 1.0))
    run_case(model, LR, "mini_free_ctrl", synth_batch(4, 12, 40, seed=4, teacher=False), controls=(1.2, 0.7, 1.3))
    run_case(model, LR, "mini_free_ctrl2", synth_batch(4, 12, 40, seed=5, teacher=False), controls=(0.8, 1.0, 0.8))
    # padding classes: one utterance, alone and beside companions that are 1, 2 and 3 phonemes longer
    base = synth_batch(3, 20, seed=6)
    run_case(model, LR, "pad_base", {k: (v[:1] if torch.is_tensor(v) else v) for k, v in base.items()} | {
        "max_src_len": int(base["src_lens"][0]), "max_mel_len": int(base["mel_lens"][0])})
    run_case(model, LR, "cfg2_checksums", synth_batch(64, 64, seed=1), save_full=False)
    run_case(model, LR, "cfg4_checksums", synth_batch(256, 16, 160, seed=1), save_full=False)
    # LR stress durations (cfg4 shape): index map only
    b4 = synth_batch(256, 16, 160, seed=1)
    im, ml = index_map(LR, b4["d_targets"], b4["max_mel_len"])
    np.savez_compressed(os.path.join(HERE, "cfg4_lr_index.npz"), d=b4["d_targets"].numpy().astype(np.int16),
                        index_map=im.astype(np.int16), mel_len=ml, max_mel_len=np.array(b4["max_mel_len"]))
    print("cfg4 lr index:", im.shape)
    train_case(FastSpeech2, pc, mc, sd)


if __name__ == "__main__":
    main(*(sys.argv[1:3]))
