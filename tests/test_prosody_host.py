"""Per-phoneme control maps, host side (no GPU): the prosody_* fixtures captured from the reference
(tests/golden/gen_golden_prosody.py) against the oracle, their distance from every discrete
decision, the C ABI of include/fs2hip_prosody.h, and the argument checks of the helper that turns a
control into a kernel argument (runtime.prosody_controls / ops.control_arg)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _common import OUT_NAMES, configs, oracle_state_dict
from _prosody import load_prosody

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_prosody.h")
CASES = ["prosody_a", "prosody_b"]
# the seeds were chosen for these (gen_golden_prosody.py): 5e-4 prediction tolerance x control <= 2,
# and (d + 1) * 5e-4 <= 6e-3 for d <= 11
EDGE_MARGIN, TIE_MARGIN = 1e-3, 6e-3


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_prosody_fixture(case):
    """The oracle broadcasts like the reference: all ten outputs bit-exact with the maps."""
    from oracle import fs2_oracle as O

    torch.set_num_threads(8)
    args, p_map, d_map, outs, z = load_prosody(case)
    pc, mc, _ = configs()
    B, L = args["texts"].shape
    assert p_map.shape == (B, L) and d_map.shape == (B, L) and p_map.dtype == d_map.dtype == torch.float32
    got = O.forward(oracle_state_dict(), mc, pc, **args, p_control=p_map, e_control=1.0, d_control=d_map)
    for name, g in zip(OUT_NAMES, got):
        ref = outs[name]
        g = g.numpy()
        assert g.shape == ref.shape and g.dtype == ref.dtype, name
        np.testing.assert_array_equal(g, ref, err_msg=f"{case}:{name}")
    im, ml = O.length_regulate_index_map(got[5], None)
    np.testing.assert_array_equal(im.numpy(), z["lr_index_map"])
    np.testing.assert_array_equal(ml.numpy(), z["lr_mel_len"])


@pytest.mark.parametrize("case,src_lens,mel_lens", [("prosody_a", [13, 13, 7], [70, 145, 67]),
                                                    ("prosody_b", [17, 14, 12], [34, 18, 42])])
def test_prosody_fixture_clear_of_decisions(case, src_lens, mel_lens):
    """Discrete outputs are compared exactly on the GPU, so the reference itself must sit clear of
    every decision boundary: scaled pitch / energy predictions >= 1e-3 from a bin edge, and
    exp(log_d) - 1 >= 6e-3 from a .5 rounding tie, at every valid position."""
    args, p_map, d_map, outs, _ = load_prosody(case)
    assert args["src_lens"].tolist() == src_lens and outs["mel_lens_out"].tolist() == mel_lens
    assert float(p_map.min()) >= 0.5 and float(p_map.max()) <= 2.0 and float(d_map.min()) >= 0.5 and \
        float(d_map.max()) <= 2.0
    sd = oracle_state_dict()
    valid = ~outs["src_masks"]
    assert valid.sum() == sum(src_lens)
    for name, bins in (("p_pred", sd["variance_adaptor.pitch_bins"]), ("e_pred", sd["variance_adaptor.energy_bins"])):
        v = outs[name].astype(np.float64)[valid]
        margin = np.abs(v[:, None] - bins.double().numpy()[None, :]).min()
        assert margin >= EDGE_MARGIN, (case, name, margin)
    d = np.exp(outs["log_d"])[valid].astype(np.float64) - 1.0
    tie = np.abs(d - np.floor(d) - 0.5).min()
    assert tie >= TIE_MARGIN, (case, tie)
    # the maps do something the scalar path cannot: fractional and zero-frame durations both occur
    dr = outs["d_rounded"][valid]
    assert (dr != np.trunc(dr)).sum() >= 10 and (np.trunc(dr) == 0).sum() >= 2
    # d_rounded is the reference formula on its own log_d, per phoneme, in f32
    ref = torch.clamp(torch.round(torch.exp(torch.from_numpy(outs["log_d"])) - 1) * d_map, min=0)
    np.testing.assert_array_equal(outs["d_rounded"], ref.numpy())


def test_prosody_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_PROSODY) and len(declared) == 6, declared
    assert not set(declared) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        fn = getattr(lib, name)  # AttributeError if not exported
        res, args = _lib.SIGNATURES_PROSODY[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # every sibling takes the scalar entry's arguments plus one pointer (the map) after the control
    text = open(HEADER).read()
    assert '#include "fs2hip.h"' in text
    for name, base in (("fs2_lr_durations_map", "fs2_lr_durations"), ("fs2_length_regulate_map", "fs2_length_regulate"),
                       ("fs2_lr_fused_proj_map", "fs2_lr_fused_proj"), ("fs2_variance_embed_map", "fs2_variance_embed"),
                       ("fs2_vp_head_map", "fs2_vp_head")):
        a, b = _lib.SIGNATURES_PROSODY[name][1], _lib.SIGNATURES[base][1]
        i = len(b) - 1 - b[::-1].index(_lib._f)  # the control: the last float argument
        assert list(a) == list(b[:i + 1]) + [_lib._p] + list(b[i + 1:]), name
        assert re.search(rf"\bint {name}\(", text), name
    import ctypes
    assert ctypes.sizeof(_lib.VpFusedMapDesc) == ctypes.sizeof(_lib.VpFusedDesc) + ctypes.sizeof(ctypes.c_void_p)
    assert _lib.VpFusedMapDesc.control_map.offset == ctypes.sizeof(_lib.VpFusedDesc)


def test_build_id_covers_prosody_header(tmp_path):
    import shutil

    from fs2amd import _lib

    assert _lib.load().fs2_build_id().decode() == _lib.source_build_id()
    # the id changes with the new header's contents (a library built before an edit is refused)
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(REPO, "include"), inc)
    same = _lib.source_build_id(_lib.CSRC, str(inc / "fs2hip.h"))
    assert same == _lib.source_build_id()
    with open(inc / "fs2hip_prosody.h", "a") as f:
        f.write("/* edited */\n")
    assert _lib.source_build_id(_lib.CSRC, str(inc / "fs2hip.h")) != same


def _va(pitch="phoneme_level", energy="phoneme_level", separate=False):
    return SimpleNamespace(pitch_feature_level=pitch, energy_feature_level=energy, separate_energy_control=separate)


def test_control_normalisation_and_argument_checks():
    from fs2amd.runtime import prosody_controls

    B, L, cpu = 3, 5, torch.device("cpu")
    # numbers stay numbers; energy follows p_control unless the switch is on
    assert prosody_controls(_va(), 1.2, 0.7, 1.3, B, L, cpu) == (1.2, 1.2, 1.3)
    assert prosody_controls(_va(separate=True), 1.2, 0.7, 1.3, B, L, cpu) == (1.2, 0.7, 1.3)
    # every broadcastable form becomes a contiguous f32 [B, L] tensor with the broadcast values
    full = torch.arange(B * L, dtype=torch.float32).view(B, L) / 7 + 0.5
    for m in (full, full[:, :1], full[:1], full[0], full[0, :1], full[0, 0], full.double(), full.to(torch.bfloat16),
              full.t().contiguous().t()):
        p, e, d = prosody_controls(_va(), m, 1.0, m, B, L, cpu)
        assert e is p and d.shape == (B, L) and p.dtype == torch.float32 and p.is_contiguous()
        assert torch.equal(p, m.float().expand(B, L)) and torch.equal(d, p)
    p, e, d = prosody_controls(_va(), full, 1.0, 1.0, B, L, cpu)
    assert p.data_ptr() == full.data_ptr() and d == 1.0  # a ready [B, L] f32 map is not copied
    # e_control: ignored by default (whatever it is), a map of its own with the switch on
    p, e, d = prosody_controls(_va(), 1.1, torch.ones(7, 7), 1.0, B, L, cpu)
    assert (p, e, d) == (1.1, 1.1, 1.0)
    p, e, d = prosody_controls(_va(separate=True), 1.1, full[:, :1], 1.0, B, L, cpu)
    assert p == 1.1 and torch.equal(e, full[:, :1].expand(B, L))
    # shapes that do not broadcast, non-float maps, maps on another device
    for bad in (torch.ones(B, L + 1), torch.ones(B + 1, L), torch.ones(B), torch.ones(1, B, L), torch.ones(2, 1),
                torch.ones(0)):
        for kw in (dict(p=bad, d=1.0), dict(p=1.0, d=bad)):
            with pytest.raises((ValueError, RuntimeError), match="broadcast"):
                prosody_controls(_va(), kw["p"], 1.0, kw["d"], B, L, cpu)
    for bad in (torch.ones(B, L, dtype=torch.int64), torch.ones(B, L, dtype=torch.int32), torch.ones(B, L) > 0):
        with pytest.raises((ValueError, RuntimeError), match="float"):
            prosody_controls(_va(), bad, 1.0, 1.0, B, L, cpu)
        with pytest.raises((ValueError, RuntimeError), match="float"):
            prosody_controls(_va(), 1.0, 1.0, bad, B, L, cpu)
    with pytest.raises((ValueError, RuntimeError), match="HIP"):
        prosody_controls(_va(), full, 1.0, 1.0, B, L, torch.device("cuda", 0))  # a CPU map for a GPU forward
    # frame-level pitch or energy: a per-phoneme pitch map has no meaning; a duration map still does
    for va in (_va(pitch="frame_level"), _va(energy="frame_level"), _va("frame_level", "frame_level")):
        with pytest.raises(ValueError, match="frame_level"):
            prosody_controls(va, full, 1.0, 1.0, B, L, cpu)
        p, e, d = prosody_controls(va, 1.2, 1.0, full, B, L, cpu)
        assert p == 1.2 and torch.equal(d, full)
    with pytest.raises(ValueError, match="frame_level"):
        prosody_controls(_va(energy="frame_level", separate=True), 1.0, full, 1.0, B, L, cpu)


def test_separate_energy_control_config_switch():
    """model config variance_adaptor.separate_energy_control: default off (the reference's quirk)."""
    import copy

    from fs2amd.model import FastSpeech2

    pc, mc, _ = configs()
    assert FastSpeech2(pc, mc).variance_adaptor.separate_energy_control is False
    mc2 = copy.deepcopy(mc)
    mc2["variance_adaptor"] = {"separate_energy_control": True}
    assert FastSpeech2(pc, mc2).variance_adaptor.separate_energy_control is True
