"""The training gradient of the 12-wave split kernel (csrc/hpe_mlp2.hip, the PRE path), tensor by tensor.

The kernel's compiled-in tanh takes its exponent's constant from the per-unit scalars (colt), dZ1 is
split through v_fma_mix_f32 (split_w8_mix), and the head phase's thread id and the shuffles' lane id
are recomputed per tile (ttid, xor32_now) — none of which the whole-gradient bars of
tests/test_gpu_mlp2_image.py would see go wrong in a small tensor: the whole-gradient max-norm is set
by dW1 and could hide a wrong dW2 or db1.  So here the gradient is held PER TENSOR (dW1, db1, dW2,
db2): the error against float64, relative to that tensor's own max |g64|, is at most 4x the exact
twin's error on that tensor + 2^-24 (the project's split-vs-exact bar, applied per tensor).  The
kernel before this file was added stayed inside that bar on every tensor of every case below, so no
tensor has a widened bar (figures in DESIGN.md).

Shapes: those of tests/test_gpu_mlp2_image.py that reach each instantiation — contiguous and general,
dropout, the runtime activation, NCB = 5 with pad columns, C_in = 88."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_mlp2_image import _Case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)   # the tests of one shape share its model, exact twin and float64 oracle
def _case(cin, F, act, dropout, side, n, yscale=1.0):
    c = _Case(cin, F, act, dropout, side, n)
    if yscale != 1.0:
        c.y = (c.y * yscale).astype(c.y.dtype)
        c.yt = torch.from_numpy(c.y.reshape(n, 3).astype(np.float32)).cuda()
    return c


def _tensors(c):
    """(name, slice) of every trained tensor in the gradient vector."""
    out = []
    for k, (o, shp) in c.eng.layout.param_index.items():
        size = int(np.prod(shp))
        if o + size <= c.eng.n_train:
            out.append((str(k), slice(o, o + size)))
    assert len(out) == 4, out
    return out


def _check_per_tensor(c, g_split, tag):
    g_exact, g64 = c.exact(), c.g64()
    for name, sl in _tensors(c):
        scale = np.abs(g64[sl]).max()
        assert scale > 0, name
        e_exact = np.abs(g_exact[sl] - g64[sl]).max() / scale
        e_split = np.abs(g_split[sl] - g64[sl]).max() / scale
        bar = 4 * e_exact + 2.0 ** -24
        print('%s %s: vs float64 exact %.3e split %.3e bar %.3e (%.2f of it)' % (tag, name, e_exact, e_split, bar, e_split / bar))
        assert e_split <= bar, (tag, name, e_split, e_exact)


CASES = [
    (96, 360, 'tanh', 0.0, 33, 17),      # contiguous, 579 tiles on 256 workgroups, ragged last tile
    (96, 360, 'tanh', 0.0, 8, 40),       # one tile per workgroup
    (96, 137, 'softsign', 0.0, 33, 16),  # NCB = 5, pad columns
    (96, 200, 'elu', 0.2, 6, 500),       # runtime activation, dropout, tiles straddling images
    (96, 360, 'tanh', 0.0, 4, 100),      # P < 32: the general instantiation
    (88, 360, 'tanh', 0.3, 8, 300),      # C_in = 88 with dropout
]


@pytest.mark.parametrize('cin,F,act,dropout,side,n', CASES)
def test_gradient_per_tensor(cin, F, act, dropout, side, n):
    c = _case(cin, F, act, dropout, side, n)
    g = c.grad()
    assert np.isfinite(g).all()
    assert (g != c.exact()).any(), 'the launch ran the exact twin'
    _check_per_tensor(c, g, 'C_in=%d F=%d %s drop %.2f side %d n %d' % (cin, F, act, dropout, side, n))


@pytest.mark.parametrize('cin,F,act,dropout,side,n', CASES)
def test_gather_bit_equal_to_contiguous(cin, F, act, dropout, side, n):
    """The identity gather index runs the general instantiation: the same arithmetic, so the same bits."""
    c = _case(cin, F, act, dropout, side, n)
    g = c.grad()
    g_gather = c.grad(idx=torch.arange(n, dtype=torch.int32, device='cuda'))
    np.testing.assert_array_equal(g, g_gather)


def test_repeatable():
    c = _case(96, 360, 'tanh', 0.0, 33, 17)
    ref = c.grad()
    assert np.isfinite(ref).all()
    for r in range(1, 20):
        g = c.grad()
        assert np.array_equal(g, ref), 'run %d differs from run 0 in %d entries' % (r, int((g != ref).sum()))


def test_large_label_errors():
    """Labels x 10: dZ2 = 2 (p - y) of mixed signs up to several hundred.  dA1 = dZ2.W2^T is fp32 all
    the way (only dZ1, scaled per unit, enters fp16 fragments), so the launch stays on the split kernel
    (the guard would hand a non-finite dW1 to the exact twin) and inside the per-tensor bars."""
    c = _case(96, 360, 'tanh', 0.0, 33, 17, 10.0)
    # (a freshly initialised model predicts within a few units of 0: the errors are the labels')
    print('labels: min %.1f max %.1f' % (c.y.min(), c.y.max()))
    assert c.y.min() < -200 and c.y.max() > 200
    g = c.grad()
    assert np.isfinite(g).all()
    assert (g != c.exact()).any(), 'the launch ran the exact twin'
    _check_per_tensor(c, g, 'labels x10')
