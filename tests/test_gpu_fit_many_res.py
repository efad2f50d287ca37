"""GPU: hpe.fit_many(..., residual_stacks=True) — residual stacks (create_model_complex and the
stacks like it, csrc/hpe_res.hip) as trials of one epoch launch (hpe_res_fit_epoch_multi: block b of
the grid trains trial b).  Every equality here is bit for bit against the same model trained alone by
Model.fit on the fused path (hpe_fit_epoch: the same kernel body on a grid of one) from the same
initial weights and seed; tests/test_gpu_res.py holds that solo kernel to the per-step path and to
the float64 oracle.  No tolerance appears anywhere: a trial's workgroup runs the same instruction
stream on the same data whether or not other trials share the launch, and nothing crosses trials."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import hpe
from hpe import _lib, keras
from hpe.callbacks import EarlyStopping
from hpe.engine import OPT_KIND
from hpe.keras import layers as kl
from util import features, labels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {'adam': keras.optimizers.Adam, 'sgd': keras.optimizers.SGD, 'adamax': keras.optimizers.Adamax}


@pytest.fixture(autouse=True)
def _default_env():
    """The batch rule under test is the default one (no HPE_FIT_FUSED in the environment)."""
    prev = os.environ.pop('HPE_FIT_FUSED', None)
    yield
    os.environ.pop('HPE_FIT_FUSED', None)
    if prev is not None:
        os.environ['HPE_FIT_FUSED'] = prev


def _complex_config(reg=1e-6, dr=1e-4, init_seed=88):
    """(model_config, initial weights) of create_model_complex of the drop-in Model-88/attention_model.py."""
    path = os.path.join(ROOT, 'head-pose-estimation-model_amd', 'Model-88', 'attention_model.py')
    spec = importlib.util.spec_from_file_location('hpe_attention_model_88_fit_many_res', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    keras.backend.clear_session()
    hpe.set_seed(init_seed)
    m = mod.create_model_complex(reg, dr)
    return m.model_config, m.weights_dict()


def _stack_config(cin=88, blocks=3, bottleneck=8, act='softsign', reg=1e-6, dr=0.1, init_seed=0):
    """create_model_complex's shape with another block count / bottleneck / activation."""
    keras.backend.clear_session()
    hpe.set_seed(init_seed)
    l2 = keras.regularizers.l2(reg)

    def conv(units, a, x):
        return kl.Conv2D(filters=units, kernel_size=1, padding='same', activation=a, kernel_regularizer=l2)(x)

    inp = keras.Input(shape=(None, None, cin))
    x = kl.SpatialDropout2D(dr)(conv(16, act, inp))
    for _ in range(blocks):
        y = kl.SpatialDropout2D(dr)(conv(16, act, x))
        y = kl.SpatialDropout2D(dr)(conv(16, act, y))
        x = kl.Activation('relu')(kl.Add()([x, y]))
    if bottleneck:
        x = kl.SpatialDropout2D(dr)(conv(bottleneck, act, x))
    m = keras.Model(inp, conv(3, None, x))
    return m.model_config, m.weights_dict()


def _mlp_config(cin=88, F=64, init_seed=0):
    """A create_model-shaped regressor (hpe_fit_epoch_multi's family)."""
    keras.backend.clear_session()
    hpe.set_seed(init_seed)
    reg = keras.regularizers.l2(0.1)
    inp = keras.Input(shape=(None, None, cin))
    h = kl.Conv2D(F, 1, activation='tanh', kernel_regularizer=reg, bias_regularizer=reg)(inp)
    m = keras.Model(inp, kl.Conv2D(3, 1, kernel_regularizer=reg, bias_regularizer=reg)(h))
    return m.model_config, m.weights_dict()


def _spec(cfg, opt='adam', lr=2.8e-4, seed=5, bs=64):
    return {'mc': cfg[0], 'w': cfg[1], 'opt': opt, 'lr': lr, 'seed': seed, 'bs': bs}


def _compiled(s):
    m = hpe.model_from_config(s['mc'], s['w'])
    m.compile(optimizer=OPT[s['opt']](learning_rate=s['lr']), loss='mse', metrics=['mae'])
    return m


def _is_res(m):
    return m._eng().program('train', 1).prog.kind == 'res'


def _solo(s, x, y, epochs, **kw):
    m = _compiled(s)
    hpe.set_seed(s['seed'])
    h = m.fit(x, y, batch_size=s['bs'], epochs=epochs, verbose=0, **kw)
    assert m._last_fit_fused is True
    return m, h


def _same(ma, ha, mb, hb, tag=''):
    wa, wb = ma.weights_dict(), mb.weights_dict()
    assert list(wa) == list(wb)
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg='%s %s' % (tag, k))
    ea, eb = ma._eng(), mb._eng()
    np.testing.assert_array_equal(ea.params_t.cpu().numpy(), eb.params_t.cpu().numpy(), err_msg=tag + ' mirror')
    assert ea.iterations == eb.iterations, tag
    assert ma.optimizer.iterations == mb.optimizer.iterations, tag
    assert (ea.m is None) == (eb.m is None), tag
    if ea.m is not None:
        np.testing.assert_array_equal(ea.m.cpu().numpy(), eb.m.cpu().numpy(), err_msg=tag + ' m')
        np.testing.assert_array_equal(ea.v.cpu().numpy(), eb.v.cpu().numpy(), err_msg=tag + ' v')
    assert ha.history == hb.history, tag
    assert ha.epoch == hb.epoch, tag


def _many_vs_solo(specs, x, y, epochs, **kw):
    ms = [_compiled(s) for s in specs]
    hs = hpe.fit_many(ms, x, y, [s['bs'] for s in specs], epochs=epochs, seeds=[s['seed'] for s in specs],
                      residual_stacks=True, **kw)
    plan = hpe.fit_many.last_plan
    assert len(hs) == len(specs)
    for i, s in enumerate(specs):
        assert ms[i]._last_fit_fused is True
        ref, href = _solo(s, x, y, epochs, **kw)
        _same(ms[i], hs[i], ref, href, 'trial %d' % i)
    assert all(f == 0 for e in plan['flags'] for f, m in zip(e, ms) if _is_res(m))
    return ms, hs, plan


def test_one_trial_ragged_last_batch():
    """n = 203 at batch 64: the last batch has 11 rows, one partly filled 16-row block, and seven
    waves add only zeros to the reduce."""
    x, y = features(203, 88, seed=1), labels(203, seed=2)
    s = _spec(_complex_config(dr=0.1), seed=7)
    ms, hs, plan = _many_vs_solo([s], x, y, 2)
    assert _is_res(ms[0])
    assert plan['launches'] == [[[0]], [[0]]]
    assert len(hs[0].history['loss']) == 2 and ms[0]._eng().iterations == 2 * 4


def test_batch_shapes_of_the_wave_loop():
    """Per-model batch sizes in one call: 1 row, one 16-row block, one block per wave (128), and 144
    (wave 0 takes a second block); then n = 129 at batch 128, whose last step has a single row."""
    x, y = features(300, 88, seed=3), labels(300, seed=4)
    cfg = _complex_config(dr=0.05)
    specs = [_spec(cfg, seed=20 + i, bs=bs, opt=o, lr=lr)
             for i, (bs, o, lr) in enumerate([(1, 'sgd', 1e-4), (16, 'adam', 2.8e-4), (128, 'adamax', 1e-3),
                                              (144, 'adam', 2.8e-4)])]
    ms, _, plan = _many_vs_solo(specs, x, y, 1)
    assert [m._eng().iterations for m in ms] == [300, 19, 3, 3]
    assert plan['launches'] == [[[0, 1, 2, 3]]]
    ms, _, _ = _many_vs_solo([_spec(cfg, seed=31, bs=128)], x[:129], y[:129], 1)
    assert ms[0]._eng().iterations == 2


TEN = [('adam', 2.8e-4, 1e-6, 1e-4), ('sgd', 2.8e-4, 1e-6, 0.3), ('adamax', 1e-3, 1e-4, 0.0),
       ('adam', 1e-3, 1e-3, 0.3), ('sgd', 1e-3, 0.0, 0.1), ('adamax', 2.8e-4, 1e-2, 0.2),
       ('adam', 5e-4, 1e-5, 0.0), ('sgd', 5e-4, 1e-2, 0.2), ('adamax', 5e-4, 1e-6, 0.3), ('adam', 2e-3, 1e-4, 0.1)]


def test_ten_trials_in_one_launch():
    x, y = features(200, 88, seed=5), labels(200, seed=6)
    specs = [_spec(_complex_config(reg=reg, dr=dr, init_seed=100 + i), opt=o, lr=lr, seed=40 + 3 * i)
             for i, (o, lr, reg, dr) in enumerate(TEN)]
    ms, _, plan = _many_vs_solo(specs, x, y, 2)
    assert all(_is_res(m) for m in ms)
    assert plan['launches'] == [[list(range(10))]] * 2
    # the trials really differ: no two end with the same first-layer kernel
    first = [next(iter(m.weights_dict().values())) for m in ms]
    assert all(not np.array_equal(first[i], first[j]) for i in range(10) for j in range(i))


def test_instances_are_grouped_and_mix_with_the_create_model_family():
    x, y = features(150, 88, seed=7), labels(150, seed=8)
    cfgs = [_stack_config(blocks=2, init_seed=1), _stack_config(blocks=3, init_seed=2),
            _stack_config(blocks=3, act='tanh', init_seed=3), _mlp_config(88, 64, init_seed=4),
            _stack_config(blocks=2, dr=0.2, init_seed=5)]
    specs = [_spec(c, seed=60 + i, opt=('adam', 'sgd', 'adamax')[i % 3], lr=(2.8e-4, 1e-3, 1e-3)[i % 3])
             for i, c in enumerate(cfgs)]
    ms, _, plan = _many_vs_solo(specs, x, y, 2)
    assert [_is_res(m) for m in ms] == [True, True, True, False, True]
    lib = _lib.load()
    hs = [m._eng().program('train', 1).h for m in ms]
    ids = [lib.hpe_res_fit_multi_instance(h) for h in hs]
    assert ids[3] == -1 and min(ids[:3]) >= 0 and len(set(ids[:3])) == 3 and ids[4] == ids[0]
    assert lib.hpe_fit_multi_instance(hs[3]) >= 0 and lib.hpe_fit_multi_instance(hs[0]) == -1
    for m, i in zip(ms, ids):   # the handle entry point and the word-stream one are the same arithmetic
        w = np.ascontiguousarray(m._eng().program('train', 1).prog.words, np.int32)
        assert lib.hpe_res_fit_multi_instance_words(w.ctypes.data_as(ctypes.c_void_p), w.size) == i
    # one launch per distinct instance and epoch: three residual-stack kernels and one create_model one
    for e in plan['launches']:
        assert sorted(sorted(l) for l in e) == [[0, 4], [1], [2], [3]]


def _clone_trials(m, x, y, count, n, bs):
    """`count` copies of m's training state as hpe_fit_trial entries sharing program, data,
    permutation and seed, plus one more copy for the solo reference."""
    eng = m._eng()
    dev = eng.device
    opt = m.optimizer
    steps = -(-n // bs)
    xd = torch.from_numpy(x.reshape(n, -1)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(n).astype(np.int32)).to(dev)
    alpha = torch.from_numpy(eng._alphas_host(opt, steps)).to(dev)
    npt = eng.n_train
    st = {'params': eng.params.repeat(count + 1, 1), 'params_t': eng.params_t.repeat(count + 1, 1),
          'm': torch.rand(count + 1, npt, device=dev)[:1].repeat(count + 1, 1) * 1e-3,
          'v': torch.rand(count + 1, npt, device=dev)[:1].repeat(count + 1, 1) * 1e-6,
          'stats': torch.zeros(count + 1, steps, 3, device=dev),
          'ws': torch.full((count + 1, 16), 7, dtype=torch.int32, device=dev),
          'keep': (xd, yd, perm, alpha)}
    h = eng.program('train', 1).h

    def trial(i):
        dp = lambda t: t[i].data_ptr()  # noqa: E731
        return _lib.FitTrial(h.value, dp(st['params']), dp(st['params_t']), dp(st['m']), dp(st['v']),
                             eng.l2.data_ptr(), eng.tpos.data_ptr(), xd.data_ptr(), yd.data_ptr(), perm.data_ptr(),
                             n, bs, OPT_KIND[opt.kind], float(opt.learning_rate), float(opt.beta_1),
                             float(opt.beta_2), float(opt.epsilon), alpha.data_ptr(), 12345, 0,
                             dp(st['stats']), 3, dp(st['ws']))
    return st, [trial(i) for i in range(count + 1)]


def test_more_trials_than_cus_at_the_c_abi():
    """300 workgroups on a card of 256 CUs (a workgroup's LDS fills a CU): the last ones wait for a
    CU.  All 300 clones of one state end byte-equal to one hpe_fit_epoch of that state."""
    lib = _lib.load()
    n, bs, count = 64, 32, 300
    m = _compiled(_spec(_complex_config(dr=0.1), opt='adam'))
    assert _is_res(m)
    x, y = features(n, 88, seed=9), labels(n, seed=10)
    st, trials = _clone_trials(m, x, y, count, n, bs)
    arr = (_lib.FitTrial * count)(*trials[:count])
    table = torch.zeros(lib.hpe_res_fit_multi_table_size(count), dtype=torch.uint8, device=m._eng().device)
    _lib.check(lib.hpe_res_fit_epoch_multi(arr, count, _lib.ptr(table), _lib.stream()), 'hpe_res_fit_epoch_multi')
    t = trials[count]
    _lib.check(lib.hpe_fit_epoch(t.prog, t.params, t.params_t, t.m, t.v, t.l2, t.tpos, t.x, t.y_true, t.perm, t.n,
                                 t.batch, t.kind, t.lr, t.beta_1, t.beta_2, t.epsilon, t.alpha, t.seed_base, t.iter0,
                                 t.stats, t.stats_stride, 0, t.workspace, _lib.stream()), 'hpe_fit_epoch')
    torch.cuda.synchronize()
    assert not torch.equal(st['params'][count], m._eng().params)      # the epoch trained something
    for k in ('params', 'params_t', 'm', 'v', 'stats'):
        got = st[k].cpu().numpy().view(np.uint8).reshape(count + 1, -1)
        assert np.array_equal(got[:count], np.broadcast_to(got[count], got[:count].shape)), k
    ws = st['ws'].cpu().numpy()
    assert (ws[:, 1] == 0).all()          # every trial's flags word, zeroed from its 7 and never raised
    assert np.isfinite(st['stats'].cpu().numpy()).all() and (st['stats'][:, :, 0] > 0).all()


def test_one_trial_multi_call_equals_hpe_fit_epoch():
    """The argument packing of the two wrappers: hpe_fit_epoch and hpe_res_fit_epoch_multi with
    n_trials = 1 run the same solo entry on a grid of one, so two clones of one state
    (create_model_complex, 100 rows at batch 64: a ragged last batch of 36) end byte-equal in
    params, mirror, m, v, the stats rows and the flags word."""
    lib = _lib.load()
    n, bs = 100, 64
    m = _compiled(_spec(_complex_config(dr=0.1), opt='adam'))
    assert _is_res(m)
    x, y = features(n, 88, seed=15), labels(n, seed=16)
    st, trials = _clone_trials(m, x, y, 1, n, bs)
    table = torch.zeros(lib.hpe_res_fit_multi_table_size(1), dtype=torch.uint8, device=m._eng().device)
    _lib.check(lib.hpe_res_fit_epoch_multi((_lib.FitTrial * 1)(trials[0]), 1, _lib.ptr(table), _lib.stream()),
               'hpe_res_fit_epoch_multi')
    t = trials[1]
    _lib.check(lib.hpe_fit_epoch(t.prog, t.params, t.params_t, t.m, t.v, t.l2, t.tpos, t.x, t.y_true, t.perm, t.n,
                                 t.batch, t.kind, t.lr, t.beta_1, t.beta_2, t.epsilon, t.alpha, t.seed_base, t.iter0,
                                 t.stats, t.stats_stride, 0, t.workspace, _lib.stream()), 'hpe_fit_epoch')
    torch.cuda.synchronize()
    assert not torch.equal(st['params'][0], m._eng().params)      # the epoch trained something
    assert (st['stats'][:, :, 0] > 0).all()
    for k in ('params', 'params_t', 'm', 'v', 'stats'):
        got = st[k].cpu().numpy().view(np.uint8).reshape(2, -1)
        assert np.array_equal(got[0], got[1]), k
    ws = st['ws'].cpu().numpy()
    assert ws[0, 1] == ws[1, 1] == 0          # the flags word, zeroed from its 7 and never raised


def test_early_stopping_at_different_epochs():
    """Patience 1, 2 and 4 with a min_delta no epoch can reach: trial i stops after epoch index
    patience_i, whatever the losses are, and is absent from the launches after that."""
    x, y = features(150, 88, seed=11), labels(150, seed=12)
    vx, vy = features(50, 88, seed=13), labels(50, seed=14)
    specs = [_spec(_complex_config(dr=0.1, init_seed=i), seed=70 + i, opt=o, lr=1e-3)
             for i, o in enumerate(['adam', 'sgd', 'adamax'])]

    def cbs():
        return [[EarlyStopping(monitor='val_loss', patience=p, min_delta=1e30, restore_best_weights=r)]
                for p, r in [(1, False), (2, True), (4, False)]]

    ms = [_compiled(s) for s in specs]
    mine = cbs()
    hs = hpe.fit_many(ms, x, y, 64, epochs=6, seeds=[s['seed'] for s in specs], validation_data=(vx, vy),
                      callbacks=mine, residual_stacks=True)
    plan = hpe.fit_many.last_plan
    assert [len(h.history['val_loss']) for h in hs] == [2, 3, 5]
    assert [c[0].stopped_epoch for c in mine] == [1, 2, 4]
    assert plan['launches'] == [[[0, 1, 2]], [[0, 1, 2]], [[1, 2]], [[2]], [[2]]]
    solo = cbs()
    for i, s in enumerate(specs):
        ref, href = _solo(s, x, y, 6, validation_data=(vx, vy), callbacks=solo[i])
        _same(ms[i], hs[i], ref, href, 'trial %d' % i)
        assert mine[i][0].best == solo[i][0].best


def test_refusals_name_the_model_and_train_nothing():
    x, y = features(400, 88, seed=15), labels(400, seed=16)
    cfg = _complex_config(dr=0.1)

    def refused(models, xx, bs, match):
        before = [m.weights_dict() for m in models]
        with pytest.raises(ValueError, match=match):
            hpe.fit_many(models, xx, y, bs, epochs=1, residual_stacks=True)
        for m, b in zip(models, before):
            a = m.weights_dict()
            for k in b:
                np.testing.assert_array_equal(a[k], b[k])
            assert m._eng().iterations == 0

    dp = _compiled(_spec(cfg))
    dp._dist = (torch.distributed, None)        # what Model.distribute() records on an initialised group
    refused([_compiled(_spec(cfg)), dp], x, 64, 'model 1.*data-parallel')
    refused([_compiled(_spec(cfg)), _compiled(_spec(cfg)), _compiled(_spec(cfg))], x, [64, 64, 300],
            'model 2.*batch 300.*HPE_FIT_FUSED=1')
    refused([_compiled(_spec(cfg))], features(400, 96, seed=17), 64, 'model 0.*channels')
    # the default keeps refusing a residual stack by name, with the message it always had
    with pytest.raises(ValueError, match='model 0.*residual-stack programs run one per launch'):
        hpe.fit_many([_compiled(_spec(cfg))], x, y, 64, epochs=1)
    # and HPE_FIT_FUSED=1 lifts the batch rule, as it does for Model.fit
    os.environ['HPE_FIT_FUSED'] = '1'
    _many_vs_solo([_spec(cfg, bs=300, seed=9)], x, y, 1)


def test_c_abi_refuses_mixed_instances_and_other_kinds():
    lib = _lib.load()
    n, bs = 64, 32
    x, y = features(n, 88, seed=18), labels(n, seed=19)
    m2 = _compiled(_spec(_stack_config(blocks=2)))
    m3 = _compiled(_spec(_stack_config(blocks=3)))
    mm = _compiled(_spec(_mlp_config(88, 64)))
    assert _is_res(m2) and _is_res(m3) and not _is_res(mm)
    s2, t2 = _clone_trials(m2, x, y, 1, n, bs)
    s3, t3 = _clone_trials(m3, x, y, 1, n, bs)
    table = torch.zeros(lib.hpe_res_fit_multi_table_size(2), dtype=torch.uint8, device=m2._eng().device)
    before = [s['params'].clone() for s in (s2, s3)]

    def einval(arr, k, word):
        assert lib.hpe_res_fit_epoch_multi(arr, k, _lib.ptr(table), _lib.stream()) == 1
        err = lib.hpe_last_error()
        assert b'hpe_res_fit_epoch_multi' in err and word in err, err

    einval((_lib.FitTrial * 2)(t2[0], t3[0]), 2, b'trial 1')
    short = _lib.FitTrial.from_buffer_copy(t2[1])
    short.stats_stride = 2
    einval((_lib.FitTrial * 2)(t2[0], short), 2, b'stats_stride')
    e = mm._eng()
    dev = e.device
    stats = torch.zeros((2, 2 + 4 * e.fit_groups()), dtype=torch.float32, device=dev)
    alpha = torch.from_numpy(e._alphas_host(mm.optimizer, 2)).to(dev)
    xd, yd, perm, _ = s2['keep']
    tm = e.fit_trial(mm.optimizer, xd, yd, perm, bs, stats, 0, alpha)
    einval((_lib.FitTrial * 2)(t2[0], tm), 2, b'trial 1')
    torch.cuda.synchronize()
    for s, b in zip((s2, s3), before):
        assert torch.equal(s['params'], b)
        assert (s['ws'].cpu().numpy() == 7).all()      # not even the workspaces were zeroed
    wm = mm.weights_dict()
    for k, v in _compiled(_spec(_mlp_config(88, 64))).weights_dict().items():
        np.testing.assert_array_equal(wm[k], v)
