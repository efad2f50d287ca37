"""The contiguous-rows instantiation of the 12-wave split training kernel (csrc/hpe_mlp2.hip
mlp2_kernel<..., CONTIG>: no gather index, P >= 32; the tile pointer carried by the loop) against
the general instantiation, the exact-fp32 twin and the float64 oracle, and the
sites of its overflow guard (the pre-split's data check, the prologue's W1 check, the flush's dW1
check).

Bars as test_gpu_parity.test_train_step_12wave_kernel: the split gradient's error against float64
(max |err| / max |g|) at most 4x the exact kernel's + 2^-24, split vs exact at most 1e-6 of max |g|,
loss sums to rtol 1e-5.  The identity index (idx = arange(n)) sends the same launch through the
general instantiation (gather staging, otherwise the same arithmetic): same products in the same
order, so bit-identical gradients."""
import numpy as np
import pytest
import torch

import hpe
from test_gpu_parity import _create_model, _data_grad64
from util import features, labels

pytestmark = pytest.mark.gpu

SEED = 5


class _Case:
    """One model and launch shape: device inputs, and the gradient under each kernel choice."""

    def __init__(self, F, act, dropout, side, n):
        from hpe import _lib
        hpe.set_seed(F)
        self.m = _create_model(F, act, dropout, 0.1)
        self.eng = self.m._eng()
        self.P, self.n = side * side, n
        assert self.eng.program('train', self.P).prog.kind == 'mlp2'
        self.x = features(n, 96, seed=F + 7, h=side, w=side)
        self.y = labels(n, seed=F + 8)
        self.xt = torch.from_numpy(self.x.reshape(n * self.P, 96)).cuda()
        self.yt = torch.from_numpy(self.y.reshape(n, 3).astype(np.float32)).cuda()
        self.inv = 1.0 / (n * self.P * 3)
        self.lib = _lib.load()

    def grad(self, xt=None, idx=None, exact=False):
        prev = self.lib.hpe_set_exact_fp32(1) if exact else None
        try:
            g = self.eng.gradient(self.xt if xt is None else xt, self.yt, self.P, idx, self.n, self.inv, seed=SEED)
            return g.cpu().numpy().copy()
        finally:
            if exact:
                self.lib.hpe_set_exact_fp32(prev)

    def check_bars(self, g_split, tag):
        eng = self.eng
        g_exact = self.grad(exact=True)
        npt = eng.n_train
        g64 = _data_grad64(self.m.model_config, self.m.weights_dict(), self.x, self.y, eng.layout, SEED)
        scale = np.abs(g64).max()
        e_exact = np.abs(g_exact[:npt] - g64).max() / scale
        e_split = np.abs(g_split[:npt] - g64).max() / scale
        d = np.abs(g_split[:npt] - g_exact[:npt]).max() / scale
        print('%s: vs float64 exact %.2e split %.2e; |split - exact| / max|g| = %.2e' % (tag, e_exact, e_split, d))
        assert e_split <= 4 * e_exact + 2.0 ** -24, (e_split, e_exact)
        assert d <= 1e-6, d
        np.testing.assert_allclose(g_split[npt:npt + 2], g_exact[npt:npt + 2], rtol=1e-5)
        return g_exact


CASES = [
    (360, 'tanh', 0.0, 96, 2),      # 576 full tiles, 2-3 per workgroup
    (360, 'tanh', 0.0, 33, 17),     # 18,513 rows: the ragged tile is a workgroup's third
    (360, 'tanh', 0.0, 8, 40),      # one tile per workgroup
    (360, 'tanh', 0.0, 6, 500),     # P = 36: tiles straddle images
    (360, 'tanh', 0.3, 8, 300),     # SpatialDropout on both layers
    (137, 'softsign', 0.0, 33, 16),  # NCB = 5: zeroed partial rows, pad columns in the last wave
    (200, 'elu', 0.2, 6, 500),      # runtime activation: keeps its pad-column selects
]


@pytest.mark.parametrize('F,act,dropout,side,n', CASES)
def test_contiguous_matches_gather_and_exact(F, act, dropout, side, n):
    c = _Case(F, act, dropout, side, n)
    g_contig = c.grad()
    idx = torch.arange(n, dtype=torch.int32, device='cuda')
    g_gather = c.grad(idx=idx)
    assert np.isfinite(g_contig).all()
    np.testing.assert_array_equal(g_contig, g_gather)
    c.check_bars(g_contig, 'F=%d %s drop %.2f side %d n %d' % (F, act, dropout, side, n))


def test_small_maps_general_instantiation():
    # P = 16 < 32: contiguous rows, but TileImg's division path -> the general instantiation
    c = _Case(360, 'tanh', 0.0, 4, 100)
    c.check_bars(c.grad(), 'F=360 tanh side 4 n 100')


@pytest.mark.parametrize('side,n', [(96, 2), (33, 17)])
def test_guard_sites(side, n):
    """A feature outside the split's data range (100, NaN, +inf) in a workgroup's first tile (the
    prologue's pre-split), in a later tile of a workgroup (the head-shadow pre-split) and in the last
    valid row (the ragged tile at 33 x 33), and a W1 entry whose scaled fp16 fragment is not finite
    (+inf, and finite values past the scale's exponent clamp: the prologue's W1 check): the
    guarded launch hands the step to the exact twin, so its gradient is the exact launch's bit for
    bit (NaNs compare equal).  In-range data stays on the split kernel."""
    c = _Case(360, 'tanh', 0.0, side, n)
    rows = n * side * side
    assert rows > 256 * 32 + 5
    g_split = c.grad()
    g_exact = c.grad(exact=True)
    assert np.isfinite(g_split).all()
    assert (g_split != g_exact).any(), 'the in-range launch ran the exact twin'
    for row in (17, 256 * 32 + 5, rows - 1):
        for val in (100.0, float('nan'), float('inf')):
            xo = c.x.reshape(rows, 96).copy()
            xo[row, 5] = val
            xot = torch.from_numpy(xo).cuda()
            got, want = c.grad(xt=xot), c.grad(xt=xot, exact=True)
            np.testing.assert_array_equal(got, want, err_msg='row %d value %r' % (row, val))
            if val == 100.0:
                assert np.isfinite(got).all()
    # the next launch is back on the split kernel
    np.testing.assert_array_equal(c.grad(), g_split)
    # one W1 entry +inf, and finite ones past the weight-side scale's exponent clamp (pow2_scale stops
    # at 2^100: from a column maximum of about 2^102 = 5.1e30 on the scaled entry's fp16 hi half is
    # infinite).  The exact kernel's gradient is finite there (a saturated tanh), so an unflagged
    # split launch, with its NaNs, cannot pass for it
    eng = c.eng
    key = [k for k, (o, shp) in eng.layout.param_index.items() if int(np.prod(shp)) == 96 * 360]
    assert len(key) == 1, key
    off = eng.layout.param_index[key[0]][0] + 7 * 360 + 11
    keep = eng.params[off].clone()
    try:
        for val in (float('inf'), 1e35, -1e31):
            eng.params[off] = val
            got, want = c.grad(), c.grad(exact=True)
            np.testing.assert_array_equal(got, want, err_msg='W1 entry %r' % val)
            if np.isfinite(val):
                assert np.isfinite(want).all(), 'W1 entry %r' % val
    finally:
        eng.params[off] = keep
    np.testing.assert_array_equal(c.grad(), g_split)


def test_repeatable():
    c = _Case(360, 'tanh', 0.0, 33, 17)
    ref = c.grad()
    assert np.isfinite(ref).all()
    for r in range(1, 20):
        g = c.grad()
        assert np.array_equal(g, ref), 'run %d differs from run 0 in %d entries' % (r, int((g != ref).sum()))
