"""GPU: one training launch of the generic row program (csrc/hpe_rowprog.hip rowprog_kernel in
training mode + reduce_kernel) against the float64 oracle's autograd gradient with the same dropout
masks, on the synthetic graphs of tests/synth_graphs.py: every activation's derivative, stand-alone
Activation layers, accumulated gradients, thin layers, LayerNormalization, the SE / MHA gate,
SeparableConv2D and the two large-program geometries, at P = 1 and on 3x3 maps, and the launch
shapes no other test reaches: more tiles than workgroups, slab counts around the reduction's
16-wide unroll, ragged last tiles in a multi-workgroup launch, a gathered batch and an image offset.

Bars.  Generic training runs exact-fp32 MFMA, so the whole gradient is held to test_gpu_res.py's
bar, max |g - g64| / max |g64| <= 1e-5.  That bar hides a wrong small tensor (a bias, a LayerNorm
beta, a thin layer) behind a large one, so every parameter tensor is also held on its own, normwise
over that tensor, to max(1e-5, 4 x the error of the same oracle evaluated in fp32 on the same
inputs) — 4 x is the project's convention for two fp32 evaluations that differ in summation order.
A tensor whose float64 gradient is identically zero (the query / key projections of single-token
attention) must come out identically zero.  The two loss sums are held to rtol 1e-5.
Measured on one MI355X, worst over all cases: whole gradient 6.2e-7; one tensor 1.18e-6 (6togj6se
conv2d_3/kernel at P = 9, where the fp32 oracle's worst tensor is 2.2e-6); every case prints its own.

The CPU half (test_compiler_synth.py) holds the compiler's lowering of the same graphs to the
oracle through the numpy emulator, so a failure here alone is the kernel's.
"""
import numpy as np
import pytest
import torch

import hpe.compiler as C
import synth_graphs as SG
from hpe import _lib
from hpe.engine import Engine
from oracle import keras_ref as K
from util import check_gradient, features, input_channels, labels

pytestmark = pytest.mark.gpu

SEED = 11


def _engine(name, P):
    mc, w = SG.build(name)
    eng = Engine(mc, w, fused=False)
    c = eng.program('train', P)
    assert c.prog.kind == 'generic'
    return mc, w, eng, c


def _ops(prog):
    w = prog.words.astype(np.int64)
    oo = int(w[C.H_OPS_OFF])
    return [w[oo + C.O_WORDS * i: oo + C.O_WORDS * (i + 1)] for i in range(int(w[C.H_NOPS]))]


def _inputs(mc, n, P, seed=3):
    c = input_channels(mc)
    side = int(round(P ** 0.5))
    assert side * side == P
    return features(n, c, seed=seed, h=side, w=side), labels(n, seed=seed + 1)


def _launch(eng, x, y, P, idx=None, img_off=0):
    n = x.shape[0] if idx is None else idx.numel()
    xt = torch.from_numpy(x.reshape(-1, x.shape[-1])).cuda()
    yt = torch.from_numpy(y.reshape(-1, 3).astype(np.float32)).cuda()
    g = eng.gradient(xt, yt, P, idx, n, 1.0 / (n * P * 3), seed=SEED, img_off=img_off)
    return g.cpu().numpy().astype(np.float64)


def _check(tag, mc, w, eng, g, x, y, img_off=0):
    return check_gradient(tag, mc, w, eng, g, x, y, SEED, img_off=img_off)


def _first_layer_spread(mc, w, x):
    """Fractions of the first layer's pre-activations below and above zero, from the oracle's own
    forward of that layer with its activation taken off."""
    import copy
    cfg = copy.deepcopy(mc)
    first = next(l for l in cfg['config']['layers'] if l['class_name'] == 'Conv2D')
    first['config']['activation'] = 'linear'
    cfg['config']['output_layers'] = [[first['name'], 0, 0]]
    z = K.Graph(cfg, w).forward(x).detach().numpy()
    return float((z < 0).mean()), float((z > 0).mean()), float(np.abs(z).max())


ACT_CASES = [n for n in SG.GRAPHS if n.startswith('act_')]
OTHER_CASES = [n for n in SG.GRAPHS if not n.startswith('act_')]
SHAPES = [(1, 203), (9, 20)]


@pytest.mark.parametrize('P,n', SHAPES)
@pytest.mark.parametrize('name', ACT_CASES)
def test_activation_gradient_vs_float64_oracle(name, P, n):
    """Every activation of hpe/layers.py, as a layer's fused epilogue (act_chain) and as an
    Activation / ReLU layer of its own (act_layers), forward and derivative, on pre-activations
    that span both signs and reach several units."""
    mc, w, eng, c = _engine(name, P)
    x, y = _inputs(mc, n, P)
    if name.startswith('act_chain'):
        neg, pos, top = _first_layer_spread(mc, w, x)
        assert neg >= 0.2 and pos >= 0.2 and top >= 4.0, (neg, pos, top)
    if name.endswith('swish'):
        assert any(int(o[C.O_EZ]) >= 0 for o in _ops(c.prog))
    if P > 1:
        assert c.prog.T % P != 0      # several images per tile, and a tile boundary inside an image
    _check('%s P=%d n=%d' % (name, P, n), mc, w, eng, _launch(eng, x, y, P), x, y)


@pytest.mark.parametrize('name,P,n', [(nm, P, n) for nm in OTHER_CASES for (P, n) in SHAPES
                                      if P == 1 or SG.GRAPHS[nm][1]])
def test_graph_gradient_vs_float64_oracle(name, P, n):
    mc, w, eng, c = _engine(name, P)
    x, y = _inputs(mc, n, P)
    if P > 1:
        assert c.prog.T % P != 0
    _check('%s P=%d n=%d' % (name, P, n), mc, w, eng, _launch(eng, x, y, P), x, y)


@pytest.mark.parametrize('name', [n for n, (_, spatial) in SG.GRAPHS.items() if not spatial])
def test_graphs_refused_on_maps(name):
    mc, w = SG.build(name)
    eng = Engine(mc, w, fused=False)
    with pytest.raises(ValueError, match=r'row-local only on 1x1 feature maps \(P == 1\)'):
        eng.program('train', 9)


def _grid_cap(c):
    return _lib.load().hpe_launch_grid(c.h, 1 << 40)


# the row-local graphs a many-tile case can afford an oracle for.  The device-scratch stack 6togj6se
# (16 waves, T = 32) has the smallest cap x T of all case graphs and is among them: its float64 and
# fp32 oracles on 2 x cap + 1 tiles take 0.2 s together
MANY_TILE_CANDIDATES = ('act_chain-tanh', 'act_layers-swish', 'residual', 'thin', 'layernorm', 'wide-gslots')


@pytest.fixture(scope='module', params=['smallest', 'residual'])
def many_tiles(request):
    """A batch on P = 15x15 maps of at least 2 x grid + 1 tiles whose last tile is ragged: every
    workgroup of the persistent grid walks several tiles and carries its dW accumulators across
    them.  'smallest': the case graph with the smallest grid_cap x T (slots in device scratch, no
    dropout); 'residual': an LDS-slot graph with dropout, so the masks' image index runs over
    tiles far from the first."""
    P = 225
    names = MANY_TILE_CANDIDATES if request.param == 'smallest' else (request.param,)
    best = None
    for name in names:
        mc, w, eng, c = _engine(name, P)
        rows = _grid_cap(c) * c.prog.T
        if best is None or rows < best[0]:
            best = (rows, name, mc, w, eng, c)
    _, name, mc, w, eng, c = best
    T, cap = c.prog.T, _grid_cap(c)
    n = -(-((2 * cap + 1) * T) // P)
    if (n * P) % T == 0:
        n += 1
    x, y = _inputs(mc, n, P, seed=8)
    return name, mc, w, eng, c, P, n, x, y


def test_more_tiles_than_workgroups(many_tiles):
    name, mc, w, eng, c, P, n, x, y = many_tiles
    rows, T = n * P, c.prog.T
    grid = _lib.load().hpe_launch_grid(c.h, rows)
    ntiles = -(-rows // T)
    print('%s: T = %d, grid = %d, %d rows = %d tiles' % (name, T, grid, rows, ntiles))
    assert ntiles >= 2 * grid + 1 and rows % T != 0
    _check('%s P=%d n=%d (%d tiles on %d workgroups)' % (name, P, n, ntiles, grid), mc, w, eng,
           _launch(eng, x, y, P), x, y)


def test_many_tile_gradient_repeatable(many_tiles):
    """Fixed summation order (per-workgroup accumulators over its tiles, then the slabs in
    reduce_kernel's order): 10 launches on identical inputs are bit-identical (race screen for the
    slab and LDS accumulators)."""
    name, mc, w, eng, c, P, n, x, y = many_tiles
    xt = torch.from_numpy(x.reshape(-1, x.shape[-1])).cuda()
    yt = torch.from_numpy(y.reshape(-1, 3)).cuda()
    inv = 1.0 / (n * P * 3)
    ref = eng.gradient(xt, yt, P, None, n, inv, seed=SEED).cpu().numpy().copy()
    for _ in range(10):
        g = eng.gradient(xt, yt, P, None, n, inv, seed=SEED).cpu().numpy()
        assert np.array_equal(g, ref)


SLAB_GRIDS = (1, 3, 4, 5, 13, 16, 17, 33)


@pytest.fixture(scope='module')
def slab_case():
    """One narrow graph and 33 x T - 5 rows; the cases take leading rows of it."""
    mc, w, eng, c = _engine('act_chain-softsign', 1)
    x, y = _inputs(mc, max(SLAB_GRIDS) * c.prog.T - 5, 1, seed=12)
    return mc, w, eng, c, x, y


@pytest.mark.parametrize('grid', SLAB_GRIDS)
def test_slab_counts_around_the_reduction_unroll(slab_case, grid):
    """grid workgroups, one tile each, the last ragged: reduce_kernel sums 1..33 slabs, through
    its 16-wide unrolled loop (grid >= 13), its tail, or both."""
    mc, w, eng, c, x, y = slab_case
    n = grid * c.prog.T - 5
    assert _lib.load().hpe_launch_grid(c.h, n) == grid
    _check('act_chain-softsign grid=%d n=%d' % (grid, n), mc, w, eng, _launch(eng, x[:n], y[:n], 1), x[:n], y[:n])


@pytest.mark.parametrize('P,n', SHAPES)
def test_gather_and_image_offset(P, n):
    """A permuted batch read through the image index (as fit gathers it) at image offset 1000
    with dropout on (a data-parallel rank's share of a batch): the oracle on the permuted rows with
    image_offset = 1000; and the offset does change the result."""
    mc, w, eng, c = _engine('act_chain-elu', P)
    n_all = n + 37
    x, y = _inputs(mc, n_all, P, seed=14)
    perm = np.random.default_rng(5).permutation(n_all)[:n].astype(np.int32)
    idx = torch.from_numpy(perm).cuda()
    g = _launch(eng, x, y, P, idx=idx, img_off=1000)     # rows and labels both read through idx
    _check('act_chain-elu gather + img_off P=%d n=%d' % (P, n), mc, w, eng, g, x[perm], y[perm], img_off=1000)
    g0 = _launch(eng, x, y, P, idx=idx, img_off=0)
    assert np.abs(g0 - g)[:eng.n_train].max() > 1e-3 * np.abs(g[:eng.n_train]).max()
