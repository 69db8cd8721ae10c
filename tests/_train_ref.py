"""Host-side references for the training-kernel tests (importable without a GPU).

* keep_mask: the dropout keep bits of csrc/train.hip (mix32, drop_key, keep4, drop_threshold)
  restated in torch int64 arithmetic masked to 32 bits. It never calls a kernel, so a wrong but
  self-consistent index hash in the kernels (a truncated row, a dropped factor) cannot hide in it.
* f32_error_floor: the error of a plain f32 evaluation of an op against its float64 evaluation,
  relative to the output scale. The hostile-statistics tests bound a kernel's error by
  max(project tolerance, 4 x this floor): the factor 4 allows another, equally accurate summation
  order; nothing in the bound comes from the kernel under test.
"""
import numpy as np
import torch

_M32 = 0xFFFFFFFF


def _mul32(x, c):
    """(x * c) mod 2^32 for an int64 tensor x in [0, 2^32) without overflowing int64."""
    lo = (x & 0xFFFF) * c
    hi = (((x >> 16) * c) & 0xFFFF) << 16
    return (lo + hi) & _M32


def mix32(x):
    """train.hip's mix32 on an int64 tensor holding uint32 values."""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def mix32_int(x):
    """The same hash on one Python int (a second, scalar statement for the host test)."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def drop_key(seed, salt):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return mix32_int((s & _M32) ^ mix32_int(((s >> 32) + (int(salt) & _M32) * 0x9E3779B9) & _M32))


def drop_threshold(p):
    """uint32(p * 2^24) with p rounded to f32 first, as the C ABI takes it; 0 switches dropout off."""
    p = float(np.float32(p))
    if not p > 0.0:
        return 0
    return min(int(p * 16777216.0), 16777216)


def keep_mask(seed, salt, n_rows, n_cols, p):
    """bool [n_rows, n_cols]: keep = (mix32((row * n_cols + col) ^ key) >> 8) >= uint32(p * 2^24)."""
    thr = drop_threshold(p)
    if thr == 0:
        return torch.ones(n_rows, n_cols, dtype=torch.bool)
    key = drop_key(seed, salt)
    idx = (torch.arange(n_rows, dtype=torch.int64)[:, None] * n_cols + torch.arange(n_cols, dtype=torch.int64)[None]) & _M32
    return (mix32(idx ^ key) >> 8) >= thr


def f32_error_floor(fn32, fn64, scale=None):
    """max |fn32() - fn64()| / scale: what a plain f32 evaluation of the op loses on this input.
    fn32 / fn64 are tensors or callables returning one; scale defaults to max |fn64()|."""
    a = fn32() if callable(fn32) else fn32
    b = fn64() if callable(fn64) else fn64
    b = b.detach().double()
    if scale is None:
        scale = float(b.abs().max())
    return float((a.detach().double() - b).abs().max()) / max(float(scale), 1e-300)
