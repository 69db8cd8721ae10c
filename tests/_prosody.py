"""Loading the per-phoneme control-map fixtures (tests/golden/prosody_*.npz, gen_golden_prosody.py)."""
import numpy as np
import torch

from _common import load_case


def load_prosody(case):
    """(args, p_map, d_map, outs, z) of a prosody fixture; the maps as f32 tensors [B, L]
    (e_control is the number 1.0; the fixture's ``controls`` holds NaN where a map stands)."""
    args, controls, outs, z = load_case(case)
    assert controls[1] == 1.0 and np.isnan(controls[0]) and np.isnan(controls[2])
    return args, torch.from_numpy(z["map_p_control"]), torch.from_numpy(z["map_d_control"]), outs, z
