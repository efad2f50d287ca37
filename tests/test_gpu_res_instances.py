"""GPU: every compiled instance of the fused residual-stack kernels (csrc/hpe_res.hip: input width
88 | 96, 1..4 blocks, with / without bottleneck, compile-time "fast" or runtime activations) against
the float64 oracle's autograd gradient with the same dropout masks, tensor by tensor, on the stacks
of tests/res_stacks.py.  tests/test_res_instances.py asserts that those stacks reach all 32
instances; tests/test_gpu_res.py holds create_model_complex alone, and only normwise over the whole
gradient, behind which a wrong bias gradient or first-layer block of an 8..11-layer stack hides.

One launch of res_train_kernel (Engine.gradient: hpe_train_step + hpe_reduce) per case: every
instance at 203 rows (13 blocks on 8 waves, the last with 11 valid rows) and on 3x3 maps; ragged and
tiny launches (1, 16, 17, 128, 129 rows); 5x5 maps (P > 16: a block inside one image or across
two); 2, 3, 5 and 17 workgroups (interleaved 16-row blocks, slabs summed by reduce_kernel, 17 past
its 16-wide unroll); a gathered batch at image offset 1000; and a 10-launch race screen of a
runtime instance.  The epoch kernel (res_fit_kernel's solo entry) of four other geometries is then
held bit for bit to the per-step path, which the cases above and tests/test_gpu_optim.py anchor.

Bars: util.check_gradient, the generic path's (tests/test_gpu_rowprog_grad.py): the kernels are
exact fp32, so whole gradient max |g - g64| / max |g64| <= 1e-5; every parameter tensor normwise
over itself within max(1e-5, 4 x the error of the same oracle in fp32 on the same inputs); a zero
float64 gradient exactly zero; both loss sums at rtol 1e-5.
Measured on one MI355X, worst over the 108 gradient cases: whole gradient 4.13e-6 (96-tanh-nb4-bot8,
n = 129); one tensor 7.85e-6 (88-tanh-nb4-bot8 conv2d/kernel at P = 1, n = 203, where the fp32
oracle's error on that tensor is 3.11e-6); the fp32 oracle's own worst tensor ranges from 1.4e-7 to
9.9e-6 over the cases, so the 4 x term does engage; every case prints its own.
"""
import os

import numpy as np
import pytest
import torch

import hpe
import res_stacks as RS
from hpe import _lib, keras
from hpe.engine import Engine
from util import check_gradient, features, labels

pytestmark = pytest.mark.gpu

SEED = 11
_ENGINES = {}


def _engine(name, P=1):
    """(model_config, weights, Engine) of a case, built once; its training program must be the
    fused residual-stack one."""
    if name not in _ENGINES:
        mc, w = RS.build(name)
        _ENGINES[name] = (mc, w, Engine(mc, w))
    mc, w, eng = _ENGINES[name]
    assert eng.program('train', P).prog.kind == 'res'
    return mc, w, eng


def _inputs(name, n, P, seed=3):
    side = int(round(P ** 0.5))
    assert side * side == P
    return features(n, RS.CASES[name]['cin'], seed=seed, h=side, w=side), labels(n, seed=seed + 1)


def _launch(eng, x, y, P, idx=None, img_off=0):
    n = x.shape[0] if idx is None else idx.numel()
    xt = torch.from_numpy(x.reshape(-1, x.shape[-1])).cuda()
    yt = torch.from_numpy(y.reshape(-1, 3).astype(np.float32)).cuda()
    g = eng.gradient(xt, yt, P, idx, n, 1.0 / (n * P * 3), seed=SEED, img_off=img_off)
    return g.cpu().numpy().astype(np.float64)


def _run(name, P, n, tag=''):
    mc, w, eng = _engine(name, P)
    x, y = _inputs(name, n, P)
    return check_gradient('%s P=%d n=%d%s' % (name, P, n, tag), mc, w, eng, _launch(eng, x, y, P), x, y, SEED)


@pytest.mark.parametrize('P,n', [(1, 203), (9, 20)])
@pytest.mark.parametrize('name', list(RS.CASES))
def test_instance_gradient_vs_float64_oracle(name, P, n):
    """Every instance and every edge stack: 203 rows are 13 blocks on 8 waves (five waves run two,
    the last block holds 11 valid rows); 20 images of 3x3 are 180 rows whose blocks straddle images,
    with dropout per image and channel."""
    _run(name, P, n)


# one fast and one runtime instance of each width; the 88-channel runtime one is an edge stack with
# dropout on every layer, the output included
RAGGED = ['88-softsign-nb2-bot8', '96-softsign-nb3-bot0', 'edge-sigmoid-bot5', '96-tanh-nb4-bot8']


@pytest.mark.parametrize('n', [1, 16, 17, 128, 129])
@pytest.mark.parametrize('name', RAGGED)
def test_ragged_and_tiny_launches(name, n):
    """n = 1 leaves seven waves and 15 lanes with nothing valid, 16 | 17 sit on the block boundary,
    128 | 129 bracket one block per wave."""
    _run(name, 1, n)


@pytest.mark.parametrize('name', ['88-softsign-nb4-bot0', 'edge-elu-bot16'])
def test_maps_wider_than_a_block(name):
    """P = 25 > 16 rows: a block lies inside one image or straddles two."""
    _run(name, 25, 7)


GRIDS = {513: 2, 1100: 3, 2555: 5, 8699: 17}
MULTI_WG = ['88-softsign-nb3-bot8', '96-tanh-nb2-bot0']


@pytest.mark.parametrize('n', list(GRIDS))
@pytest.mark.parametrize('name', MULTI_WG)
def test_several_workgroups(name, n):
    """More than 512 rows: ceil(n / 512) workgroups take interleaved 16-row blocks and reduce_kernel
    sums their slabs.  513 puts one valid row in the second workgroup; 17 slabs pass the reduction's
    16-wide unroll."""
    mc, w, eng = _engine(name)
    assert RS.CASES[name]['dr'] > 0
    assert _lib.load().hpe_launch_grid(eng.program('train', 1).h, n) == GRIDS[n] == -(-n // 512)
    _run(name, 1, n, ' (%d workgroups)' % GRIDS[n])


@pytest.mark.parametrize('P,n', [(1, 203), (9, 20)])
@pytest.mark.parametrize('name', ['88-softsign-nb1-bot8', '96-tanh-nb3-bot8'])
def test_gather_and_image_offset(name, P, n):
    """A permuted batch read through the image index (as fit gathers it) at image offset 1000 (a
    chunk or a data-parallel rank's share of a batch) under dropout: the oracle on the permuted rows
    with image_offset = 1000; and the offset does change the result."""
    mc, w, eng = _engine(name, P)
    assert RS.CASES[name]['dr'] > 0
    n_all = n + 37
    x, y = _inputs(name, n_all, P, seed=14)
    perm = np.random.default_rng(5).permutation(n_all)[:n].astype(np.int32)
    idx = torch.from_numpy(perm).cuda()
    g = _launch(eng, x, y, P, idx=idx, img_off=1000)     # rows and labels both read through idx
    check_gradient('%s gather + img_off P=%d n=%d' % (name, P, n), mc, w, eng, g, x[perm], y[perm], SEED,
                   img_off=1000)
    g0 = _launch(eng, x, y, P, idx=idx, img_off=0)
    assert np.abs(g0 - g)[:eng.n_train].max() > 1e-3 * np.abs(g[:eng.n_train]).max()


def test_runtime_instance_gradient_repeatable():
    """Fixed summation order (8-wave tree, slabs in reduce_kernel's order): 10 launches of a runtime
    instance on three workgroups are bit-identical (race screen; test_gpu_res.py screens the
    canonical fast instance)."""
    name, n = '96-tanh-nb2-bot0', 1100
    mc, w, eng = _engine(name)
    x, y = _inputs(name, n, 1, seed=6)
    xt = torch.from_numpy(x.reshape(n, -1)).cuda()
    yt = torch.from_numpy(y.reshape(n, 3)).cuda()
    ref = eng.gradient(xt, yt, 1, None, n, 1.0 / (n * 3), seed=SEED).cpu().numpy().copy()
    assert np.abs(ref[:eng.n_train]).max() > 0
    for _ in range(10):
        g = eng.gradient(xt, yt, 1, None, n, 1.0 / (n * 3), seed=SEED).cpu().numpy()
        assert np.array_equal(g, ref)


OPT = {'sgd': lambda: keras.optimizers.SGD(learning_rate=2.8e-4),
       'adam': lambda: keras.optimizers.Adam(learning_rate=2.8e-4),
       'adamax': lambda: keras.optimizers.Adamax(learning_rate=1e-3)}


@pytest.mark.parametrize('name,opt', [('96-softsign-nb1-bot0', 'sgd'), ('88-tanh-nb4-bot8', 'adam'),
                                      ('edge-sigmoid-bot5', 'adamax'), ('edge-softplus-nobias', 'adam')])
def test_fused_epoch_matches_per_step_bit_for_bit(name, opt):
    """fit's whole-epoch launch (res_fit_kernel<.., false>) of geometries other than
    create_model_complex's against the per-step path (res_train_kernel on one workgroup +
    hpe_reduce_optim_step): 200 rows at batch 64 (a last batch of 8), 2 shuffled epochs, every
    weight bit-identical.

    The no-bias softplus stack found a bug here: its tanh post-add saturates, the data gradient
    (~1e-5) is smaller than the l2 term, and res_opt_one's g + 2 c2 w had been contracted into
    fma(2 c2, w, g) while the per-step optimizer rounds the product first, so a fifth of the first
    step's Adam moments differed in the last bit and one word of conv2d/kernel after 8 steps."""
    mc, w = RS.build(name, reg=1e-4)
    x = features(200, RS.CASES[name]['cin'], seed=21)
    y = labels(200, seed=22)
    out, hist = {}, {}
    prev = os.environ.get('HPE_FIT_FUSED')
    try:
        for mode in ('0', '1'):
            os.environ['HPE_FIT_FUSED'] = mode
            hpe.set_seed(5)
            m = hpe.model_from_config(mc, w)
            m.compile(optimizer=OPT[opt](), loss='mse', metrics=['mae'])
            assert m._eng().program('train', 1).prog.kind == 'res'
            h = m.fit(x, y, batch_size=64, epochs=2, shuffle=True, verbose=0)
            assert m._last_fit_fused == (mode == '1')
            out[mode] = m.weights_dict()
            hist[mode] = h.history['loss']
    finally:
        if prev is None:
            os.environ.pop('HPE_FIT_FUSED', None)
        else:
            os.environ['HPE_FIT_FUSED'] = prev
    assert list(out['0']) == list(out['1']) == list(w)
    for k, v in out['0'].items():
        assert np.isfinite(v).all() and not np.array_equal(v, w[k]), k     # trained, not diverged
        np.testing.assert_array_equal(out['1'][k], v, err_msg=k)
    np.testing.assert_allclose(hist['1'], hist['0'], rtol=1e-5)
