"""The row-swapped fp16 image of the 12-wave split training kernel (csrc/hpe_mlp2.hip img_row,
presplit_tile, tr_read8): tile row r is stored at image row img_row(r) (bits 0-1 <-> bits 2-3), the
forward reads its row there, and dW1's transposed reads address the swapped rows.  Launches from
32,768 rows on run the library's second object of the kernel, which also reads dz2 packed ([T][3]): the
large-launch cases below are the ones that reach it.

A row that the forward and the transposed reader place differently would pair one row's X with another
row's dZ1.  Whole random tiles can hide that behind the max-norm of a large gradient, so the first test
lights ONE tile row at a time: X is zero except tile row r0, every row's dZ1 is live (the loss gradient
does not vanish on a zero row), and dW1 = X^T dZ1 is right only if row r0's X meets row r0's dZ1.

Bars as tests/test_gpu_mlp2_bwd_mfma.py, per tensor (dW1, db1, dW2, db2): the error against float64,
relative to the tensor's max |g64|, at most 4x the exact twin's + 2^-24.  The image paths run at the
smallest shapes tests/test_gpu_mlp2_image.py names for them.  tests/test_lds_image_swap.py models the
addressing and the banks on the CPU."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_mlp2_bwd_mfma import _check_per_tensor, _tensors
from test_gpu_mlp2_image import SEED, _Case
from test_gpu_parity import _data_grad64

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(cin, F, act, dropout, side, n):
    return _Case(cin, F, act, dropout, side, n)


def _one_hot(cin, side, n):
    """X zero except the rows r with r % 32 == r0, for each r0 in 0..31; the exact twin's gradient and
    the float64 oracle's are computed here for each input (the case's own caches are not used)."""
    c = _Case(cin, 360, 'tanh', 0.0, side, n)
    rows = n * side * side
    live = c.x.reshape(rows, cin).copy()
    assert (np.abs(live).max(axis=1) > 0).all()     # every row has something to show
    for r0 in range(32):
        x = np.zeros((rows, cin), np.float32)
        x[r0::32] = live[r0::32]
        c.x = x.reshape(n, side, side, cin)
        c.xt = torch.from_numpy(x).cuda()
        g, g_exact = c.grad(), c.grad(exact=True)
        g64 = _data_grad64(c.m.model_config, c.m.weights_dict(), c.x, c.y, c.eng.layout, SEED)
        assert np.isfinite(g).all(), r0
        assert (g != g_exact).any(), 'row %d: the launch ran the exact twin' % r0
        for name, sl in _tensors(c):
            scale = np.abs(g64[sl]).max()
            assert scale > 0, (r0, name)
            e_exact = np.abs(g_exact[sl] - g64[sl]).max() / scale
            e_split = np.abs(g[sl] - g64[sl]).max() / scale
            bar = 4 * e_exact + 2.0 ** -24
            print('C_in=%d rows %d one-hot row %d %s: exact %.3e split %.3e bar %.3e' % (cin, rows, r0, name, e_exact, e_split, bar))
            assert e_split <= bar, (r0, name, e_split, e_exact)


@pytest.mark.parametrize('cin', [96, 88])
def test_one_hot_rows(cin):
    """One 6 x 6 image: 36 rows, one full tile and a ragged one; X zero except tile row r0."""
    _one_hot(cin, 6, 1)


def test_one_hot_rows_large_launch():
    """The same on a launch past MLP2_BIG_ROWS (32,768 rows), which runs the library's second object of
    the kernel (other compiler flags): 31 images of 33 x 33 = 1,089 rows (33,759 rows: tile rows and image
    rows drift apart, the last tile is ragged)."""
    _one_hot(96, 33, 31)


PATHS = [
    (96, 360, 'tanh', 0.0, 33, 17),      # three tiles on one workgroup, ragged last tile: both parities, one reused
    (96, 360, 'tanh', 0.0, 8, 40),       # one tile per workgroup: the prologue's pre-split only
    (96, 137, 'softsign', 0.0, 33, 16),  # NCB = 5, pad columns
    (96, 360, 'tanh', 0.0, 4, 100),      # P < 32: the general instantiation
    (96, 360, 'tanh', 0.0, 33, 31),      # 33,759 rows: past MLP2_BIG_ROWS, the library's second object of the kernel
]


@pytest.mark.parametrize('cin,F,act,dropout,side,n', PATHS)
def test_image_paths_per_tensor(cin, F, act, dropout, side, n):
    c = _case(cin, F, act, dropout, side, n)
    g = c.grad()
    assert np.isfinite(g).all()
    assert (g != c.exact()).any(), 'the launch ran the exact twin'
    _check_per_tensor(c, g, 'C_in=%d F=%d %s side %d n %d' % (cin, F, act, side, n))


@pytest.mark.parametrize('cin,F,act,dropout,side,n', PATHS)
def test_identity_gather_bit_equal(cin, F, act, dropout, side, n):
    c = _case(cin, F, act, dropout, side, n)
    g = c.grad()
    g_gather = c.grad(idx=torch.arange(n, dtype=torch.int32, device='cuda'))
    np.testing.assert_array_equal(g, g_gather)


def test_repeatable():
    c = _case(96, 360, 'tanh', 0.0, 33, 17)
    ref = c.grad()
    assert np.isfinite(ref).all()
    for r in range(1, 10):
        g = c.grad()
        assert np.array_equal(g, ref), 'run %d differs from run 0 in %d entries' % (r, int((g != ref).sum()))
