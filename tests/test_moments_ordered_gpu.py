"""satrl_moments_ordered: the sums of x and x^2 added in a fixed order, so a
run and its resumed copy normalise their advantages and report their
explained variance with the same bits.  Checked bit for bit against a numpy
restatement of that order, at one block, at block edges, at three blocks (the
checkpoint tests' 96 x 8 table) and past the 1024-block grid cap."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 255, 256, 257, 768, 1000, 256 * 1024 + 77]


def _tree(v):
    """The xor-shuffle tree over a wave's 64 lanes, then the block's waves in order."""
    v = v.reshape(-1, 64).T.copy()                 # [lane, wave]
    off = 32
    while off:
        v = v[:off] + v[off:2 * off]
        off >>= 1
    out = np.float64(0.0)
    for w in range(v.shape[1]):
        out = out + v[0, w]
    return out


def _ordered(x):
    n = x.size
    blocks = min((n + 255) // 256, 1024)
    xd = x.astype(np.float64)
    part = np.zeros((2, blocks))
    for k, vals in enumerate((xd, xd * xd)):
        pad = np.zeros(-(-n // (blocks * 256)) * blocks * 256)
        pad[:n] = vals
        rows = pad.reshape(-1, blocks, 256)        # [grid-stride pass, block, thread]
        acc = np.zeros((blocks, 256))
        for r in rows:                             # each thread adds its elements in index order
            acc = acc + r
        part[k] = [_tree(acc[b]) for b in range(blocks)]
    out = np.zeros(2)
    for k in range(2):
        acc = np.zeros(256)
        for j in range(0, blocks, 256):            # thread t adds part[t], part[t + 256], ...
            chunk = np.zeros(256)
            chunk[:min(256, blocks - j)] = part[k, j:j + 256]
            acc = acc + chunk
        out[k] = 0.0 + _tree(acc)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_moments_ordered_is_the_stated_order(n):
    from satrl.ppo import moments
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3)).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    got = moments(xt).cpu().numpy()
    want = _ordered(x)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    for _ in range(3):                             # the same bits on every call
        assert np.array_equal(moments(xt).cpu().numpy(), got)
    acc = torch.tensor([1.5, -2.0], dtype=torch.float64, device="cuda")       # out accumulates
    assert np.array_equal(moments(xt, out=acc).cpu().numpy(), np.array([1.5, -2.0]) + want)


def test_moments_ordered_refuses_a_small_scratch():
    import satrl._lib as L
    lib = L.lib()
    assert lib.satrl_moments_scratch(0) == -1 and lib.satrl_moments_scratch(256) == 2
    assert lib.satrl_moments_scratch(257) == 4 and lib.satrl_moments_scratch(1 << 30) == 2048
    fake = C.c_void_p(16)                          # never touched: refused before any launch
    assert lib.satrl_moments_ordered(768, fake, fake, fake, 5, None) == -1
    assert b"scratch holds 5" in lib.satrl_last_error()
    assert lib.satrl_moments_ordered(768, fake, fake, None, 6, None) == -1
    assert lib.satrl_moments_ordered(0, fake, fake, fake, 6, None) == -1
