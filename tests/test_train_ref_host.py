"""tests/_train_ref.py on the CPU: the host statement of the training kernels' dropout hash and the
f32 error floor behave as the GPU tests assume."""
import pytest
import torch
import torch.nn.functional as F

import _train_ref as TR

SEED_HI = (0x1234ABCD << 32) | 0x9E3779B1  # non-zero high 32 bits


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [1234567, SEED_HI])
def test_keep_fraction(p, seed):
    k = TR.keep_mask(seed, 7, 9223, 256, p)
    assert k.shape == (9223, 256) and k.dtype == torch.bool
    assert abs(float(k.float().mean()) - (1 - p)) < 0.01 * (1 - p)
    # no row or column structure: every row and every column keeps about 1 - p
    # (binomial, 6 sigma: 6 * sqrt(p (1 - p) / n))
    assert float((k.float().mean(1) - (1 - p)).abs().max()) < 6 * (p * (1 - p) / 256) ** 0.5
    assert float((k.float().mean(0) - (1 - p)).abs().max()) < 6 * (p * (1 - p) / 9223) ** 0.5


def test_masks_differ_across_seed_and_salt():
    base = TR.keep_mask(5, 3, 64, 256, 0.3)
    assert torch.equal(base, TR.keep_mask(5, 3, 64, 256, 0.3))
    for seed, salt in ((6, 3), (5, 4), (5 | (1 << 32), 3), (5 | (1 << 63), 3)):
        other = TR.keep_mask(seed, salt, 64, 256, 0.3)
        frac = float((other != base).float().mean())
        assert abs(frac - 2 * 0.3 * 0.7) < 0.03, (seed, salt, frac)  # independent masks differ on 2 p (1 - p)


def test_threshold_edges():
    assert TR.drop_threshold(0.0) == 0 and TR.drop_threshold(-1.0) == 0
    assert TR.drop_threshold(0.5) == 1 << 23
    assert TR.drop_threshold(0.1) == 1677721  # uint32(float(0.1f) * 2^24)
    assert TR.drop_threshold(1.0) == 1 << 24
    assert bool(TR.keep_mask(99, 1, 37, 80, 0.0).all())
    assert not bool(TR.keep_mask(99, 1, 37, 80, 1.0).any())  # (h >> 8) < 2^24 always


def test_tensor_hash_equals_scalar_hash():
    """The int64-tensor arithmetic (split multiplies, no int64 overflow) equals plain Python
    integers mod 2^32, on the index range of the tests and at the uint32 edges."""
    xs = [0, 1, 255, 256, 9222 * 256 + 255, 3332 * 80 + 79, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF]
    got = TR.mix32(torch.tensor(xs, dtype=torch.int64)).tolist()
    assert got == [TR.mix32_int(x) for x in xs]
    key = TR.drop_key(SEED_HI, 11)
    assert key != TR.drop_key(SEED_HI & 0xFFFFFFFF, 11)  # the high word enters the key
    k = TR.keep_mask(SEED_HI, 11, 50, 80, 0.5)
    for r, c in ((0, 0), (1, 0), (49, 79), (17, 33)):
        assert bool(k[r, c]) == ((TR.mix32_int((r * 80 + c) ^ key) >> 8) >= (1 << 23))


def test_row_factor_matters():
    """row * n_cols + col: masks of different widths differ, and rows are not copies of row 0."""
    k = TR.keep_mask(3, 2, 8, 256, 0.5)
    assert not any(torch.equal(k[0], k[r]) for r in range(1, 8))
    assert torch.equal(TR.keep_mask(3, 2, 2, 512, 0.5).view(4, 256), TR.keep_mask(3, 2, 4, 256, 0.5))


def test_error_floor():
    torch.manual_seed(0)
    x = torch.randn(64, 256) + 1e3
    f = lambda t: F.layer_norm(t, (256,))
    floor = TR.f32_error_floor(lambda: f(x), lambda: f(x.double()))
    assert 1e-7 < floor < 1e-3  # mean 1e3 / std 1 costs f32 about 1e3 * 2^-24 / std
    plain = torch.randn(64, 256)
    assert TR.f32_error_floor(f(plain), f(plain.double())) < 2e-6
    assert TR.f32_error_floor(plain, plain.double(), scale=2.0) == 0.0
