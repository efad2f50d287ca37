"""The 12-wave split training kernel on ONE fp16 image per X tile (csrc/hpe_mlp2.hip presplit_tile,
img_pos, tr_read8): the forward reads the image by rows, dW1 reads the same image transposed with
ds_read_b64_tr_b16, and the image has two parities (tile t + 1 is split while tile t's backward reads).

Bars as test_gpu_mlp2_contig: the split gradient's error against float64 (max |err| / max |g|) at most
4x the exact kernel's + 2^-24, split vs exact at most 1e-6 of max |g|, loss sums to rtol 1e-5, and the
identity gather index (the general instantiation, otherwise the same arithmetic) bit-equal to the
contiguous launch.  Shapes: the smallest that reach each path of the image — both parities and a
parity reused by a workgroup's third tile with a ragged last tile (579 tiles on 256 workgroups), one
tile per workgroup (the prologue's pre-split only), NCB = 5 with pad columns, the runtime activation
with tiles straddling images, P < 32 (the general instantiation), and C_in = 88, where the image has
its gap at position 44 and dW1's third channel block reads the zeroed pad positions.

tests/test_lds_image_tr.py models the image's addressing and banking on the CPU."""
import functools

import numpy as np
import pytest
import torch

import hpe
from hpe import keras
from test_gpu_parity import _create_model, _data_grad64
from util import features, labels

pytestmark = pytest.mark.gpu

SEED = 5


def _model88(F, act, dropout):
    """88-channel input (Model-88's BlazeFace tap) on a width the 12-wave kernel takes."""
    keras.backend.clear_session()
    reg = keras.regularizers.l2(1e-6)
    inp = keras.Input(shape=(None, None, 88))
    h = keras.layers.Conv2D(F, 1, padding='same', activation=act, kernel_regularizer=reg)(inp)
    h = keras.layers.SpatialDropout2D(dropout)(h)
    o = keras.layers.Conv2D(3, 1, padding='same', kernel_regularizer=reg)(h)
    o = keras.layers.SpatialDropout2D(dropout)(o)
    m = keras.Model(inp, o)
    m.compile(optimizer=keras.optimizers.Adam(learning_rate=2.8e-4), loss='mse', metrics=['mae'])
    return m


class _Case:
    """One model and launch shape: device inputs, and the gradient under each kernel choice; the
    exact twin's gradient and the float64 oracle's computed once."""

    def __init__(self, cin, F, act, dropout, side, n):
        from hpe import _lib
        hpe.set_seed(F + cin)
        self.m = _create_model(F, act, dropout, 0.1) if cin == 96 else _model88(F, act, dropout)
        self.eng = self.m._eng()
        self.cin, self.P, self.n = cin, side * side, n
        assert self.eng.program('train', self.P).prog.kind == 'mlp2'
        self.x = features(n, cin, seed=F + 7, h=side, w=side)
        self.y = labels(n, seed=F + 8)
        self.xt = torch.from_numpy(self.x.reshape(n * self.P, cin)).cuda()
        self.yt = torch.from_numpy(self.y.reshape(n, 3).astype(np.float32)).cuda()
        self.inv = 1.0 / (n * self.P * 3)
        self.lib = _lib.load()
        self._exact = self._g64 = None

    def grad(self, idx=None, exact=False):
        prev = self.lib.hpe_set_exact_fp32(1) if exact else None
        try:
            g = self.eng.gradient(self.xt, self.yt, self.P, idx, self.n, self.inv, seed=SEED)
            return g.cpu().numpy().copy()
        finally:
            if exact:
                self.lib.hpe_set_exact_fp32(prev)

    def exact(self):
        if self._exact is None:
            self._exact = self.grad(exact=True)
        return self._exact

    def g64(self):
        if self._g64 is None:
            self._g64 = _data_grad64(self.m.model_config, self.m.weights_dict(), self.x, self.y, self.eng.layout, SEED)
        return self._g64

    def check_bars(self, g_split, tag):
        npt = self.eng.n_train
        g_exact, g64 = self.exact(), self.g64()
        scale = np.abs(g64).max()
        e_exact = np.abs(g_exact[:npt] - g64).max() / scale
        e_split = np.abs(g_split[:npt] - g64).max() / scale
        d = np.abs(g_split[:npt] - g_exact[:npt]).max() / scale
        print('%s: vs float64 exact %.2e split %.2e; |split - exact| / max|g| = %.2e' % (tag, e_exact, e_split, d))
        assert e_split <= 4 * e_exact + 2.0 ** -24, (e_split, e_exact)
        assert d <= 1e-6, d
        np.testing.assert_allclose(g_split[npt:npt + 2], g_exact[npt:npt + 2], rtol=1e-5)


@functools.lru_cache(maxsize=1)   # the last case built: consecutive tests of one shape share it
def _case(cin, F, act, dropout, side, n):
    return _Case(cin, F, act, dropout, side, n)


CASES = [
    (96, 360, 'tanh', 0.0, 33, 17),      # 579 tiles: both parities, parity 0 again for a third tile, ragged last tile
    (96, 360, 'tanh', 0.0, 8, 40),       # one tile per workgroup: the prologue's pre-split only
    (96, 137, 'softsign', 0.0, 33, 16),  # NCB = 5, pad columns
    (96, 200, 'elu', 0.2, 6, 500),       # runtime activation, tiles straddling images
    (96, 360, 'tanh', 0.0, 4, 100),      # P < 32: the general instantiation
    (88, 160, 'softsign', 0.0, 33, 17),  # the gap at 44, pad channels 88..95, NCB = 5
    (88, 360, 'tanh', 0.3, 8, 300),      # the same, with dropout
    (88, 360, 'tanh', 0.0, 33, 17),      # the same at full width (shared with the pad-accumulator test)
]


@pytest.mark.parametrize('cin,F,act,dropout,side,n', CASES)
def test_one_image_matches_exact_and_gather(cin, F, act, dropout, side, n):
    c = _case(cin, F, act, dropout, side, n)
    g = c.grad()
    assert np.isfinite(g).all()
    g_gather = c.grad(idx=torch.arange(n, dtype=torch.int32, device='cuda'))
    np.testing.assert_array_equal(g, g_gather)
    c.check_bars(g, 'C_in=%d F=%d %s drop %.2f side %d n %d' % (cin, F, act, dropout, side, n))


def test_pad_accumulators_read_zeros():
    """C_in = 88: dW1's third channel block covers channels 64..95, and the accumulators of the pad
    channels 88..95 are part of the flush's overflow check.  They read the image's zeroed positions;
    anything else there (stale LDS: possibly NaN or inf) could set the guard and hand the launch to
    the exact twin.  A finite, in-range launch stays on the split kernel: its gradient differs from
    the exact twin's somewhere."""
    c = _case(88, 360, 'tanh', 0.0, 33, 17)
    g_split = c.grad()
    assert np.isfinite(g_split).all()
    assert (g_split != c.exact()).any(), 'the in-range launch ran the exact twin'


def test_repeatable():
    c = _case(96, 360, 'tanh', 0.0, 33, 17)
    ref = c.grad()
    assert np.isfinite(ref).all()
    for r in range(1, 20):
        g = c.grad()
        assert np.array_equal(g, ref), 'run %d differs from run 0 in %d entries' % (r, int((g != ref).sum()))
