"""The 12-wave split training kernel with the W2 rows of its head partials handed to the FMAs by DPP row
broadcast (csrc/hpe_mlp2.hip BCH, csrc/hpe_dev.h fmac3x4_bcast; the library's large-launch object): a
lane of the wave holds ONE table entry, and `row_newbcast:N` picks the entry of lane N of the reader's
16-lane row.  A wrong lane map pairs a unit's activation with another unit's W2 row.  (The same was
built for the backward's dZ2 rows and measured slower; the cases that would catch a row's
activation meeting another row's dZ2 stay: they hold the shipped table reads as well.)

Bars of tests/test_gpu_mlp2_bwd_mfma.py, per tensor (dW1, db1, dW2, db2): the error against float64,
relative to the tensor's max |g64|, at most 4x the exact twin's on that tensor + 2^-24.

Shapes: F = 136 (five waves: the narrowest 12-wave launch, the last wave has 8 units) and F = 360;
C_in 96 and 88; 37 rows at P = 37 (one full tile and a ragged one); 32,768 + 5 rows, from which the
library's large-launch object of the kernel runs; gathered batches; SpatialDropout on layer 1 and on
the output (the head's division path) and without.  Random W2 rows differ per unit and the rows' dZ2
differ per row; two structured cases make a swap impossible to cancel: W2 zero except ONE unit, and
the loss error confined to ONE tile row (P = 1: each row has its own label; the rows r with
r % 32 != r0 get a label equal to their prediction, bit for bit).  The structured cases leave a tensor
with one live unit or one live row per tile, so its error no longer averages over units or tile rows
as the bars, set on dense gradients, presuppose (the split kernel's tanh alone is 2^-22 absolute,
csrc/hpe_dev.h): they run on 1,089 rows, 34 tiles and a ragged one, which average in their place.
tests/test_dpp_tables.py models the two lane maps on the CPU, tests/test_gpu_bcast_probe.py holds the
instruction."""
import functools

import numpy as np
import pytest
import torch

import hpe
from test_gpu_mlp2_bwd_mfma import _check_per_tensor, _tensors
from test_gpu_mlp2_image import _Case, _model88
from test_gpu_parity import _create_model
from util import features, labels

pytestmark = pytest.mark.gpu

BIG = 32768 + 5     # = 13 * 2521 rows: past MLP2_BIG_ROWS, ragged last tile


class _Rows(_Case):
    """_Case on h x 1 images (P = h rows per image, not a square)."""

    def __init__(self, cin, F, act, dropout, h, n):
        from hpe import _lib
        hpe.set_seed(F + cin)
        self.m = _create_model(F, act, dropout, 0.1) if cin == 96 else _model88(F, act, dropout)
        self.eng = self.m._eng()
        self.cin, self.P, self.n = cin, h, n
        assert self.eng.program('train', self.P).prog.kind == 'mlp2'
        self.x = features(n, cin, seed=F + 7, h=h, w=1)
        self.y = labels(n, seed=F + 8)
        self.xt = torch.from_numpy(self.x.reshape(n * self.P, cin)).cuda()
        self.yt = torch.from_numpy(self.y.reshape(n, 3).astype(np.float32)).cuda()
        self.inv = 1.0 / (n * self.P * 3)
        self.lib = _lib.load()
        self._exact = self._g64 = None

    def set_labels(self, y):
        self.y = np.ascontiguousarray(y, np.float32)
        self.yt = torch.from_numpy(self.y.reshape(self.n, 3)).cuda()
        self._exact = self._g64 = None

    def weights(self):
        """(W1 [C_in][F], b1 [F], W2 [F][3], b2 [3]) and their keys, by the layout's order."""
        w = self.m.weights_dict()
        keys = [k for k, (o, shp) in sorted(self.eng.layout.param_index.items(), key=lambda kv: kv[1][0])
                if o + int(np.prod(shp)) <= self.eng.n_train]
        assert len(keys) == 4, keys
        return keys, [np.asarray(w[k]) for k in keys]

    def set_weight(self, key, a):
        self.eng.set_weights({key: a})
        np.testing.assert_array_equal(self.m.weights_dict()[key], a)
        self._exact = self._g64 = None


@functools.lru_cache(maxsize=None)
def _case(cin, F, act, dropout, h, n):
    return _Rows(cin, F, act, dropout, h, n)


def _split_within_bars(c, tag, idx=None):
    g = c.grad(idx=idx)
    assert np.isfinite(g).all(), tag
    assert (g != c.exact()).any(), '%s: the launch ran the exact twin' % tag
    _check_per_tensor(c, g, tag)
    return g


CASES = [
    (96, 136, 'tanh', 0.0, 37, 1),        # 37 rows at P = 37, five waves, last wave 8 units
    (96, 360, 'tanh', 0.0, 37, 1),
    (88, 136, 'softsign', 0.0, 37, 1),
    (88, 360, 'tanh', 0.0, 37, 1),
    (96, 136, 'tanh', 0.0, 37, 3),        # three images: tiles straddle them (and a real gather below)
    (96, 136, 'tanh', 0.25, 37, 3),       # dropout on layer 1 and on the output: the head's divisions
    (88, 360, 'softsign', 0.25, 37, 3),
    (96, 360, 'elu', 0.25, 37, 3),        # the runtime-activation instantiation
    (96, 360, 'tanh', 0.0, 2521, 13),     # 32,768 + 5 rows: the large-launch object
    (88, 136, 'tanh', 0.25, 2521, 13),
]


@pytest.mark.parametrize('cin,F,act,dropout,h,n', CASES)
def test_gradient_per_tensor(cin, F, act, dropout, h, n):
    c = _case(cin, F, act, dropout, h, n)
    assert n * h in (37, 111, BIG)
    tag = 'C_in=%d F=%d %s drop %.2f P %d n %d' % (cin, F, act, dropout, h, n)
    g = _split_within_bars(c, tag)
    # the identity gather runs the general instantiation: the same arithmetic, the same bits
    np.testing.assert_array_equal(g, c.grad(idx=torch.arange(n, dtype=torch.int32, device='cuda')))


@pytest.mark.parametrize('cin,F,act,dropout,h,n', [c for c in CASES if c[5] > 1 and c[3] == 0.0])
def test_gathered_batch(cin, F, act, dropout, h, n):
    """A real permutation of the images (no dropout: the sum over rows is the same set in float64)."""
    c = _case(cin, F, act, dropout, h, n)
    perm = np.roll(np.arange(n), 1)[::-1].copy()
    assert (perm != np.arange(n)).any()
    _split_within_bars(c, 'gathered C_in=%d F=%d P %d n %d' % (cin, F, h, n),
                       idx=torch.from_numpy(perm.astype(np.int32)).cuda())


@pytest.mark.parametrize('cin,F,h,n', [(96, 136, 37, 1), (96, 360, 2521, 13)])
def test_repeatable(cin, F, h, n):
    c = _case(cin, F, 'tanh', 0.0, h, n)
    ref = c.grad()
    assert np.isfinite(ref).all()
    for r in range(1, 20):
        g = c.grad()
        assert np.array_equal(g, ref), 'run %d differs from run 0 in %d entries' % (r, int((g != ref).sum()))


def _one_hot_w2(cin, F, h, n, units):
    """dW1 (column n0), dW2 (dense: every unit's A1 meets the rows' dZ2) and db2 are held to the bars as
    they stand.  db1 is ONE number here (dA1 is zero off unit n0), and a max-norm bar on one fp32 number
    is a bar on its own rounding: both kernels sum ~1,000 rounded terms in their own order, and where the
    exact twin happens to land within a tenth of an ulp (it did: 3.6e-9 at unit 135, 1,089 rows) the bar
    collapses to 2^-24, half an ulp, which no fp32 sum in another order can promise — the kernel before
    the broadcast tables missed it with the same bits (8.4e-8 against 7.4e-8).  So for this one-number
    tensor the twin's error counts as at least the format's half ulp, 2^-24; its other entries must be
    exactly zero."""
    c = _Rows(cin, F, 'tanh', 0.0, h, n)
    keys, (w1, b1, w2, b2) = c.weights()
    assert w2.shape[-2:] == (F, 3), w2.shape
    for n0 in units:
        hot = np.zeros_like(w2)
        hot[..., n0, :] = (1.5, -2.0, 0.75)
        c.set_weight(keys[2], hot)
        tag = 'C_in=%d F=%d rows %d W2 one-hot in unit %d' % (cin, F, n * h, n0)
        g = c.grad()
        assert np.isfinite(g).all(), tag
        g_exact, g64 = c.exact(), c.g64()
        assert (g != g_exact).any(), '%s: the launch ran the exact twin' % tag
        for name, sl in _tensors(c):
            scale = np.abs(g64[sl]).max()
            assert scale > 0, (tag, name)
            e_exact = np.abs(g_exact[sl] - g64[sl]).max() / scale
            e_split = np.abs(g[sl] - g64[sl]).max() / scale
            if name == str(keys[1]):
                dead = np.arange(F) != n0
                assert not g[sl][dead].any() and not g64[sl][dead].any(), (tag, name)
                e_exact = max(e_exact, 2.0 ** -24)
            bar = 4 * e_exact + 2.0 ** -24
            print('%s %s: vs float64 exact %.3e split %.3e bar %.3e' % (tag, name, e_exact, e_split, bar))
            assert e_split <= bar, (tag, name, e_split, e_exact)


def test_one_hot_w2_every_lane():
    """W2 zero except unit n0: the prediction, dA1 and dW1's only live column hang on unit n0's A1 meeting
    unit n0's W2 row.  Every lane position of a wave (wave 1), the first unit, and the last wave's last."""
    _one_hot_w2(96, 136, 1089, 1, list(range(32, 64)) + [0, 135])


def test_one_hot_w2_large_launch():
    _one_hot_w2(96, 360, 2521, 13, [5, 16 + 32 * 7 + 9, 359])


def _check_live_tensors(c, g, tag, dead):
    """_check_per_tensor on the tensors the construction leaves live; the `dead` ones are exactly zero."""
    g_exact, g64 = c.exact(), c.g64()
    for name, sl in _tensors(c):
        scale = np.abs(g64[sl]).max()
        if name in dead:
            assert scale == 0 and not g[sl].any() and not g_exact[sl].any(), (tag, name)
            continue
        assert scale > 0, (tag, name)
        e_exact = np.abs(g_exact[sl] - g64[sl]).max() / scale
        e_split = np.abs(g[sl] - g64[sl]).max() / scale
        bar = 4 * e_exact + 2.0 ** -24
        print('%s %s: vs float64 exact %.3e split %.3e bar %.3e' % (tag, name, e_exact, e_split, bar))
        assert e_split <= bar, (tag, name, e_split, e_exact)


def _one_tile_row_error(F, rows, r0s):
    """P = 1 (a label per row) and a prediction that is b2 in every row whatever the arithmetic, so with
    the labels at b2 a row's dZ2 is exactly zero; the rows r0, r0 + 32, ... get another label.  Two ways
    to pin the prediction:
      * W2 = 0: dW2 = A1^T dZ2 and db2 are live (row r0's A1 must meet row r0's dZ2), dW1 = db1 = 0;
      * W1 = 0, b1 = 0 (A1 = tanh(0) = 0 in the split kernel, the exact one and float64): dA1 = dZ2.W2^T,
        dW1 = X^T dZ1 and db1 are live (row r0's X must meet row r0's dZ2), dW2 = 0."""
    c = _Rows(96, F, 'tanh', 0.0, 1, rows)
    keys, (w1, b1, w2, b2) = c.weights()
    names = [str(k) for k in keys]
    for zero, dead in (((2,), (names[0], names[1])), ((0, 1), (names[2],))):
        for i, a in enumerate((w1, b1, w2, b2)):
            c.set_weight(keys[i], np.zeros_like(a) if i in zero else a)
        for r0 in r0s:
            y = np.tile(b2.reshape(1, 3), (rows, 1)).astype(np.float32)
            live = np.arange(r0, rows, 32)
            y[live] += (labels(rows, seed=F + r0)[live] + np.float32([30.0, -20.0, 10.0]))
            c.set_labels(y)
            g = c.grad()
            assert np.isfinite(g).all()
            assert (g != c.exact()).any(), 'the launch ran the exact twin'
            _check_live_tensors(c, g, 'F=%d rows %d zeroed %s error in tile row %d' % (F, rows, zero, r0), dead)


def test_one_tile_row_error_every_row():
    _one_tile_row_error(136, 1089, list(range(32)))


def test_one_tile_row_error_large_launch():
    _one_tile_row_error(360, BIG, [21, 4])
