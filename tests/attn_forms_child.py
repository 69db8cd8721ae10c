"""Child process of tests/test_gpu_attention_forms.py::test_env_only_forms (a helper, not
collected by pytest). FS2_ATTN32 and FS2_ATTN32_FORM are read into statics once per process, so
the kernel forms only they reach (attn_bf16_kernel<8,2>, attn32_kernel<8,3>) need a process of
their own; the parent sets one of them in this child's environment.

Runs the T = 449 bf16 case table with waves = 8, padded and packed, every score family, with
lse, and prints one JSON line of the per-case errors (the parent asserts the bounds). The first
HIP error or failed launch raises, so the process exits non-zero without starting the next case."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO, os.path.join(REPO, "expressive-fastspeech2-mandarin_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"


def main():
    import _attn_cases as A

    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device")
    res = {}
    for family in A.FAMILIES:
        c = A.make_case(family, "t449", 2, "bf16")
        for packed in (False, True):
            out, lse, _ = A.launch(c, DEV, packed, waves=8, lse=True)
            err, at = A.seq_rel_err(out, c.ref, c.lens, c.T, packed)
            res[f"{family}/{'packed' if packed else 'padded'}"] = dict(
                err=err, at=at, lse=A.lse_err(lse, c.lse, c.lens, c.T, packed))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
