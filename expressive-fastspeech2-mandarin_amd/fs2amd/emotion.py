"""Host helpers that build the weights ``FastSpeech2.forward`` / ``SynthGraphs`` take in place of
speaker / emotion / arousal / valence ids (runtime.cond_inputs): a row of weights over the rows of
an embedding table per utterance ([B, n]) or, for the three emotion inputs, per phoneme
([B, max_src_len, n]). Pure torch on the CPU; move the result to the model's device. The
dictionaries are those of ``<preprocessed_path>/emotions.json`` / ``speakers.json`` (name -> row).

    w_e = mixture({"Happy": .7, "Neutral": .3}, emotion_dict)        # 70 % happy
    w_a = level_weights(0.65, arousal_dict)                          # between the levels 0.5 and 0.8
    ramp = curve([(0, mixture({"Neutral": 1}, emotion_dict)), (L - 1, mixture({"Angry": 1}, emotion_dict))], L, L)

Weights are used as given (not normalised): a sum above 1 raises the intensity, a negative entry
extrapolates away from a row. They must be finite.
"""
import torch


def one_hot(ids, n):
    """ids (int, sequence or integer tensor of any shape) -> f32 [..., n] one-hot rows."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise ValueError(f"one_hot: id outside [0, {n})")
    return torch.nn.functional.one_hot(ids, n).to(torch.float32)


def mixture(weights, dictionary):
    """{name: weight} over ``dictionary`` (name -> row) -> f32 [n] weight row; names that are not
    mentioned get 0. An unknown name raises KeyError."""
    row = torch.zeros(len(dictionary), dtype=torch.float32)
    for name, w in weights.items():
        if name not in dictionary:
            raise KeyError(f"mixture: {name!r} is not in the dictionary ({sorted(dictionary)})")
        row[dictionary[name]] += float(w)
    return row


def level_weights(value, dictionary):
    """A number on the scale of a dictionary whose keys are numbers (the arousal levels "0.3" ..
    "0.9") -> f32 [n]: piecewise-linear weights on the two neighbouring levels, one-hot at a level
    and beyond either end."""
    levels = sorted((float(k), int(r)) for k, r in dictionary.items())
    row = torch.zeros(len(dictionary), dtype=torch.float32)
    v = float(value)
    if v <= levels[0][0]:
        row[levels[0][1]] = 1.0
        return row
    if v >= levels[-1][0]:
        row[levels[-1][1]] = 1.0
        return row
    for (lo, r_lo), (hi, r_hi) in zip(levels[:-1], levels[1:]):
        if lo <= v <= hi:
            t = (v - lo) / (hi - lo)
            row[r_lo] += 1.0 - t
            row[r_hi] += t
            return row
    raise ValueError(f"level_weights: {value!r} is not a number on the scale")


def curve(keyframes, src_len, L):
    """[(phoneme index, weight row [n]), ...] -> f32 [L, n]: the rows interpolated linearly between
    keyframes, constant before the first and after the last keyframe; positions from ``src_len`` on
    (padding, which the model still adds a vector to) repeat position src_len - 1."""
    if not keyframes:
        raise ValueError("curve: at least one keyframe")
    keys = sorted(((int(i), torch.as_tensor(r, dtype=torch.float32)) for i, r in keyframes), key=lambda k: k[0])
    if any(a[0] == b[0] for a, b in zip(keys[:-1], keys[1:])):
        raise ValueError("curve: two keyframes at one phoneme index")
    if not 1 <= int(src_len) <= int(L):
        raise ValueError(f"curve: src_len {src_len} outside [1, L = {L}]")
    n = keys[0][1].numel()
    out = torch.empty(int(L), n, dtype=torch.float32)
    for i in range(int(L)):
        p = min(i, int(src_len) - 1)
        if p <= keys[0][0]:
            out[i] = keys[0][1]
        elif p >= keys[-1][0]:
            out[i] = keys[-1][1]
        else:
            for (i0, r0), (i1, r1) in zip(keys[:-1], keys[1:]):
                if i0 <= p <= i1:
                    t = (p - i0) / (i1 - i0)
                    out[i] = (1.0 - t) * r0 + t * r1
                    break
    return out
