"""GPU: hpe.fit_many — independent trials side by side in one epoch launch (hpe_fit_epoch_multi,
csrc/hpe_fit.hip).  Every trial is compared with the same model trained alone by Model.fit on the
fused path (HPE_FIT_FUSED=1) from the same initial weights and seed.  The comparison is bit
equality: a trial's workgroups run the same instruction stream on the same data whether or not
other trials share the launch, the cross-workgroup sum is in fixed workgroup order, and nothing
crosses trials.  One case anchors the chain to the float64 oracle."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import hpe
from hpe import _lib, keras
from hpe.callbacks import EarlyStopping
from oracle import keras_ref as K
from util import features, fixture, labels

pytestmark = pytest.mark.gpu

OPT = {'adam': keras.optimizers.Adam, 'sgd': keras.optimizers.SGD, 'adamax': keras.optimizers.Adamax}


@pytest.fixture(autouse=True)
def _fused_env():
    prev = os.environ.get('HPE_FIT_FUSED')
    os.environ['HPE_FIT_FUSED'] = '1'
    yield
    if prev is None:
        os.environ.pop('HPE_FIT_FUSED', None)
    else:
        os.environ['HPE_FIT_FUSED'] = prev


def _config(F=64, act='tanh', dropout=0.0, l2=0.1, cin=96, init_seed=0):
    """(model_config, initial weights) of a create_model-shaped regressor."""
    keras.backend.clear_session()
    hpe.set_seed(init_seed)
    reg = keras.regularizers.l2(l2)
    inp = keras.Input(shape=(None, None, cin))
    h = keras.layers.Conv2D(F, 1, activation=act, kernel_regularizer=reg, bias_regularizer=reg)(inp)
    h = keras.layers.SpatialDropout2D(dropout)(h)
    o = keras.layers.Conv2D(3, 1, kernel_regularizer=reg, bias_regularizer=reg)(h)
    o = keras.layers.SpatialDropout2D(dropout)(o)
    m = keras.Model(inp, o)
    return m.model_config, m.weights_dict()


def _compiled(spec):
    m = hpe.model_from_config(spec['mc'], spec['w'])
    m.compile(optimizer=OPT[spec.get('opt', 'adam')](learning_rate=spec.get('lr', 2.8e-4)), loss='mse',
              metrics=['mae'])
    return m


def _spec(opt='adam', lr=2.8e-4, seed=5, bs=128, **kw):
    mc, w = _config(**kw)
    return {'mc': mc, 'w': w, 'opt': opt, 'lr': lr, 'seed': seed, 'bs': bs}


def _solo(spec, x, y, epochs, fused=True, **kw):
    m = _compiled(spec)
    os.environ['HPE_FIT_FUSED'] = '1' if fused else '0'
    try:
        hpe.set_seed(spec['seed'])
        h = m.fit(x, y, batch_size=spec['bs'], epochs=epochs, verbose=0, **kw)
    finally:
        os.environ['HPE_FIT_FUSED'] = '1'
    return m, h


def _same(ma, ha, mb, hb, tag=''):
    wa, wb = ma.weights_dict(), mb.weights_dict()
    assert list(wa) == list(wb)
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg='%s %s' % (tag, k))
    ea, eb = ma._eng(), mb._eng()
    assert ea.iterations == eb.iterations, tag
    assert ma.optimizer.iterations == mb.optimizer.iterations, tag
    assert (ea.m is None) == (eb.m is None), tag
    if ea.m is not None:
        np.testing.assert_array_equal(ea.m.cpu().numpy(), eb.m.cpu().numpy(), err_msg=tag + ' m')
        np.testing.assert_array_equal(ea.v.cpu().numpy(), eb.v.cpu().numpy(), err_msg=tag + ' v')
    assert ha.history == hb.history, tag
    assert ha.epoch == hb.epoch, tag


def _many_vs_solo(specs, x, y, epochs, **kw):
    """fit_many over specs, each compared with its solo run; returns (models, histories)."""
    ms = [_compiled(s) for s in specs]
    hs = hpe.fit_many(ms, x, y, [s['bs'] for s in specs], epochs=epochs, seeds=[s['seed'] for s in specs], **kw)
    plan = hpe.fit_many.last_plan
    assert len(hs) == len(specs)
    for i, s in enumerate(specs):
        assert ms[i]._last_fit_fused is True
        ref, href = _solo(s, x, y, epochs, **{k: v for k, v in kw.items() if k != 'callbacks'})
        assert ref._last_fit_fused is True
        _same(ms[i], hs[i], ref, href, 'trial %d' % i)
    hpe.fit_many.last_plan = plan
    return ms, hs


def _device_launches(models):
    """Launches per epoch hpe_fit_multi_plan gives for these trials (one instance) on this device."""
    lib = _lib.load()
    cap = lib.hpe_fit_multi_lane_cap(models[0]._eng().program('train', 1).h)
    groups = [m._eng().fit_groups() for m in models]
    count, rest = 0, groups
    while rest:
        n = len(rest)
        k = lib.hpe_fit_multi_plan((ctypes.c_int32 * n)(*rest), n, cap, (ctypes.c_int32 * n)(),
                                   (ctypes.c_int32 * n)())
        assert k >= 1
        rest = rest[k:]
        count += 1
    return count, cap


def test_one_trial_equals_fit():
    x, y = features(300, 96, seed=1), labels(300, seed=2)
    _many_vs_solo([_spec(F=64, dropout=0.2, seed=7)], x, y, 2)
    assert [len(e) for e in hpe.fit_many.last_plan['launches']] == [1, 1]


EIGHT = [dict(opt=o, lr=lr, seed=11 + i, dropout=d, l2=l2, init_seed=i)
         for i, (o, lr, d, l2) in enumerate([('adam', 2.8e-4, 0.0, 0.1), ('adamax', 1e-3, 0.2, 0.05),
                                             ('sgd', 0.01, 0.0, 0.1), ('adam', 1e-3, 0.2, 0.01),
                                             ('adamax', 2.8e-4, 0.0, 0.05), ('sgd', 0.02, 0.2, 0.1),
                                             ('adam', 5e-4, 0.2, 0.2), ('adamax', 5e-4, 0.0, 0.01)])]


@pytest.fixture(scope='module')
def eight():
    os.environ['HPE_FIT_FUSED'] = '1'
    x, y = features(300, 96, seed=3), labels(300, seed=4)
    specs = [_spec(F=64, **kw) for kw in EIGHT]
    ms = [_compiled(s) for s in specs]
    hs = hpe.fit_many(ms, x, y, 128, epochs=2, seeds=[s['seed'] for s in specs])
    return specs, x, y, ms, hs, hpe.fit_many.last_plan


def test_eight_trials_equal_their_solo_runs(eight):
    specs, x, y, ms, hs, plan = eight
    assert [len(e) for e in plan['launches']] == [1, 1]     # one instance, one launch per epoch
    assert sorted(plan['launches'][0][0]) == list(range(8))
    for i, s in enumerate(specs):
        ref, href = _solo(s, x, y, 2)
        _same(ms[i], hs[i], ref, href, 'trial %d' % i)


def test_two_of_the_eight_match_the_oracle(eight):
    """The equality chain is anchored to the reference semantics, not only to our solo path: the
    float64 oracle's step-by-step fit (as test_gpu_fit._oracle_fit), that file's tolerances."""
    specs, x, y, ms, hs, plan = eight
    for i in (1, 3):    # Adamax and Adam, both with dropout 0.2
        s = specs[i]
        g = K.Graph(s['mc'], s['w'])
        o = K.LegacyOptimizer(s['opt'], s['lr'])
        rng = np.random.RandomState(s['seed'])
        it = 0
        for e in range(2):
            p = rng.permutation(len(x))
            for b0 in range(0, len(p), 128):
                it += 1
                b = p[b0:b0 + 128]
                K.train_step(g, o, x[b], y[b], drop_seed=(s['seed'] * 1000003 + it) & 0xFFFFFFFFFFFFFFFF)
        w = ms[i].weights_dict()
        for k in g.trainable:
            np.testing.assert_allclose(w[k], g.params[k].detach().numpy(), rtol=2e-4, atol=2e-5,
                                       err_msg='trial %d %s' % (i, k))


def test_mixed_widths_in_one_launch():
    x, y = features(301, 96, seed=5), labels(301, seed=6)     # ragged last batch: 301 = 2 * 128 + 45
    specs = [_spec(F=F, seed=20 + i, dropout=0.1 * (i % 2), init_seed=i) for i, F in enumerate([16, 64, 100, 384])]
    ms, _ = _many_vs_solo(specs, x, y, 2)
    assert [m._eng().fit_groups() for m in ms] == [1, 2, 4, 12]
    assert [len(e) for e in hpe.fit_many.last_plan['launches']] == [1, 1]


@pytest.mark.parametrize('F,count', [(100, 11), (384, 20)])
def test_stacked_trials(F, count):
    x, y = features(200, 96, seed=7), labels(200, seed=8)
    specs = [_spec(F=F, seed=30 + i, dropout=0.2 * (i % 2), init_seed=i % 3,
                   opt=('adam', 'sgd', 'adamax')[i % 3], lr=(2.8e-4, 0.01, 1e-3)[i % 3]) for i in range(count)]
    ms, _ = _many_vs_solo(specs, x, y, 2)
    plan = hpe.fit_many.last_plan
    want, cap = _device_launches(ms)
    assert [len(e) for e in plan['launches']] == [want, want]
    if cap == 32:   # MI355X: 256 CUs at one workgroup each
        assert want == (1 if F == 100 else 2)
    assert sorted(i for launch in plan['launches'][0] for i in launch) == list(range(count))


def test_per_model_batch_sizes_and_big_batch():
    x, y = features(400, 96, seed=9), labels(400, seed=10)
    specs = [_spec(F=64, seed=40 + i, bs=bs, dropout=0.1, init_seed=i) for i, bs in enumerate([32, 128, 200])]
    # batch 512 (> 256): the partial table overlays the X slots and X is re-gathered for the backward
    specs.append(_spec(F=100, seed=44, bs=512, init_seed=4))
    _many_vs_solo(specs, x, y, 2)


def test_kernel_instances_are_grouped():
    mc, w = fixture('stoqa9pt')     # Model-88: 88 -> 64 softsign -> 3
    x88, y = features(300, 88, seed=11), labels(300, seed=12)
    s88 = [{'mc': mc, 'w': w, 'opt': 'adam', 'lr': 2.8e-4, 'seed': 50 + i, 'bs': 128} for i in range(2)]
    _many_vs_solo(s88, x88, y, 2)
    assert [len(e) for e in hpe.fit_many.last_plan['launches']] == [1, 1]
    x96 = features(300, 96, seed=13)
    specs = [_spec(F=64, act=a, seed=60 + i, dropout=0.1, init_seed=i) for i, a in enumerate(['tanh', 'relu', 'elu'])]
    _many_vs_solo(specs, x96, y, 2)
    # tanh has its own instance; relu and elu share the runtime-activation one
    launches = hpe.fit_many.last_plan['launches']
    assert [sorted(sorted(l) for l in e) for e in launches] == [[[0], [1, 2]]] * 2


def _oracle_val_losses(s, x, y, vx, vy, epochs):
    g = K.Graph(s['mc'], s['w'])
    o = K.LegacyOptimizer(s['opt'], s['lr'])
    rng = np.random.RandomState(s['seed'])
    it, out = 0, []
    for e in range(epochs):
        p = rng.permutation(len(x))
        for b0 in range(0, len(p), s['bs']):
            it += 1
            b = p[b0:b0 + s['bs']]
            K.train_step(g, o, x[b], y[b], drop_seed=(s['seed'] * 1000003 + it) & 0xFFFFFFFFFFFFFFFF)
        pred = g.forward(vx).detach().numpy().reshape(-1, 3)
        out.append(float(((pred - vy.reshape(-1, 3)) ** 2).mean() + float(g.regularization())))
    return out


def _stops_after(vals, patience, min_delta):
    """Index of the epoch after which EarlyStopping stops on this val_loss sequence, or None."""
    cb = EarlyStopping(monitor='val_loss', patience=patience, min_delta=min_delta)

    class M:
        stop_training = False
    cb.set_model(M())
    cb.on_train_begin()
    for e, v in enumerate(vals):
        cb.on_epoch_end(e, {'val_loss': v})
        if cb.model.stop_training:
            return e
    return None


def test_early_stopping_at_different_epochs():
    x, y = features(300, 96, seed=14), labels(300, seed=15)
    vx, vy = features(80, 96, seed=16), labels(80, seed=17)
    specs = [_spec(F=64, seed=70 + i, lr=lr, init_seed=i) for i, lr in enumerate([2.8e-4, 1e-2, 1e-2])]
    # trial 0 learns slowly: its val_loss improves by less than min_delta from epoch 1 to 2, so with
    # patience 1 it stops after epoch 2 of 5; min_delta comes from the float64 oracle's sequence, far
    # enough (a factor 2 each way) that fp32 rounding cannot move the decision
    seq = [_oracle_val_losses(s, x, y, vx, vy, 5) for s in specs]
    d01 = seq[0][0] - seq[0][1]
    assert d01 > 0
    md = 2.0 * d01
    assert _stops_after(seq[0], 1, md) == 1
    for i in (1, 2):    # the others improve by more than 2 md every epoch or have the patience to go on
        assert _stops_after(seq[i], 5, 0.0) is None

    def cbs():
        return [[EarlyStopping(monitor='val_loss', patience=1, min_delta=md, restore_best_weights=True)],
                [EarlyStopping(monitor='val_loss', patience=5, restore_best_weights=True)],
                [EarlyStopping(monitor='val_loss', patience=5, restore_best_weights=True)]]

    ms = [_compiled(s) for s in specs]
    mine = cbs()
    hs = hpe.fit_many(ms, x, y, 128, epochs=5, seeds=[s['seed'] for s in specs], validation_data=(vx, vy),
                      callbacks=mine)
    assert [len(h.history['val_loss']) for h in hs] == [2, 5, 5]
    assert mine[0][0].stopped_epoch == 1
    np.testing.assert_allclose(hs[0].history['val_loss'], seq[0][:2], rtol=1e-3)
    solo_cbs = cbs()
    for i, s in enumerate(specs):
        ref, href = _solo(s, x, y, 5, validation_data=(vx, vy), callbacks=solo_cbs[i])
        _same(ms[i], hs[i], ref, href, 'trial %d' % i)
        assert mine[i][0].stopped_epoch == solo_cbs[i][0].stopped_epoch
        assert mine[i][0].best == solo_cbs[i][0].best


def test_shared_overflow_reruns_every_trial_exactly():
    x, y = features(300, 96, seed=9), labels(300, seed=10)
    x[17, 0, 0, 5] = 100.0      # beyond the fp16 split's data range, as in test_gpu_fit
    specs = [_spec(F=F, seed=80 + i, init_seed=i) for i, F in enumerate([64, 64, 100])]
    ms, _ = _many_vs_solo(specs, x, y, 2)
    plan = hpe.fit_many.last_plan
    for e in range(2):
        assert all(f & 1 for f in plan['flags'][e]), plan['flags']
        assert plan['exact'][e] == [0, 1, 2]
        assert len(plan['launches'][e]) == 2     # the split launch and the exact re-run
    for m in ms:
        assert all(np.isfinite(v).all() for v in m.weights_dict().values())


def test_timeout_rolls_every_trial_back_to_per_step():
    x, y = features(400, 96, seed=21), labels(400, seed=22)
    specs = [_spec(F=F, seed=90 + i, init_seed=i, dropout=0.1 * i) for i, F in enumerate([64, 100, 64])]
    ms = [_compiled(s) for s in specs]
    os.environ['HPE_FIT_FORCE_TIMEOUT'] = '1'
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            hs = hpe.fit_many(ms, x, y, 128, epochs=2, seeds=[s['seed'] for s in specs])
    finally:
        os.environ.pop('HPE_FIT_FORCE_TIMEOUT')
    assert sum('timed out' in str(w.message) for w in rec) == 3
    plan = hpe.fit_many.last_plan
    assert all(f & 2 for f in plan['flags'][0]) and plan['launches'][1] == []
    for i, s in enumerate(specs):
        assert ms[i]._last_fit_fused is False and ms[i]._eng()._fit_disabled
        ref, href = _solo(s, x, y, 2, fused=False)
        wa, wb = ms[i].weights_dict(), ref.weights_dict()
        for k in wa:
            np.testing.assert_array_equal(wa[k], wb[k], err_msg='trial %d %s' % (i, k))
        np.testing.assert_allclose(hs[i].history['loss'], href.history['loss'], rtol=1e-6)
        assert ms[i]._eng().iterations == ref._eng().iterations == 2 * 4


def test_refusals_name_the_model_and_train_nothing():
    x, y = features(100, 96, seed=23), labels(100, seed=24)
    good = _spec(F=64, seed=1)

    def refused(models, xx, match):
        before = [m.weights_dict() for m in models]
        with pytest.raises(ValueError, match=match):
            hpe.fit_many(models, xx, y, 64, epochs=1)
        for m, b in zip(models, before):
            a = m.weights_dict()
            for k in b:
                np.testing.assert_array_equal(a[k], b[k])

    raw = hpe.model_from_config(good['mc'], good['w'])          # not compiled
    refused([_compiled(good), raw], x, 'model 1.*compiled')
    mc, w = fixture('stoqa9pt')                                  # 88 channels on 96-channel data
    narrow = _compiled({'mc': mc, 'w': w})
    refused([_compiled(good), _compiled(good), narrow], x, 'model 2.*channels')
    os.environ['HPE_FIT_FUSED'] = '0'
    try:
        refused([_compiled(good)], x, 'model 0.*HPE_FIT_FUSED=0')
    finally:
        os.environ['HPE_FIT_FUSED'] = '1'


def _cin(m):
    return m._config['layers'][0]['config']['batch_input_shape'][-1]


def _residual_stack():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, 'head-pose-estimation-model_amd', 'Model-88', 'attention_model.py')
    spec = importlib.util.spec_from_file_location('hpe_attention_model_88_fit_many', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    keras.backend.clear_session()
    hpe.set_seed(88)
    m = mod.create_model_complex(1e-6, 1e-4)
    m.compile(optimizer=keras.optimizers.Adam(learning_rate=2.8e-4), loss='mse')
    return m


def test_residual_stack_is_refused_by_name():
    res = _residual_stack()
    x, y = features(100, _cin(res), seed=26), labels(100, seed=27)
    w0 = res.weights_dict()
    with pytest.raises(ValueError, match='model 0.*residual'):
        hpe.fit_many([res], x, y, 64, epochs=1)
    for k, v in res.weights_dict().items():
        np.testing.assert_array_equal(v, w0[k])


def test_c_abi_refuses_mixed_and_residual_launches():
    """hpe_fit_multi_supported / hpe_fit_epoch_multi: one kernel instance per launch, no residual
    stacks; a refused call returns HPE_EINVAL (1) and launches nothing."""
    import torch
    lib = _lib.load()
    x, y = features(100, 96, seed=30), labels(100, seed=31)
    ms = [_compiled(_spec(F=64, act=a, init_seed=i)) for i, a in enumerate(['tanh', 'tanh', 'relu'])]
    dev = ms[0]._eng().device
    xd = torch.from_numpy(x.reshape(100, 96)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    perm = torch.arange(100, dtype=torch.int32, device=dev)
    keep = []

    def trial(m):
        e = m._eng()
        stats = torch.zeros((1, 2 + 4 * e.fit_groups()), dtype=torch.float32, device=dev)
        alpha = torch.from_numpy(e._alphas_host(m.optimizer, 1)).to(dev)
        keep.extend([stats, alpha])
        return e.fit_trial(m.optimizer, xd, yd, perm, 128, stats, 0, alpha)

    same = (_lib.FitTrial * 2)(trial(ms[0]), trial(ms[1]))
    mixed = (_lib.FitTrial * 2)(trial(ms[0]), trial(ms[2]))
    assert lib.hpe_fit_multi_supported(same, 2) == 1
    assert lib.hpe_fit_multi_supported(mixed, 2) == 0
    assert lib.hpe_fit_multi_instance(ms[0]._eng().program('train', 1).h) != \
        lib.hpe_fit_multi_instance(ms[2]._eng().program('train', 1).h) >= 0
    table = torch.zeros(lib.hpe_fit_multi_table_size(2), dtype=torch.uint8, device=dev)
    before = [m.weights_dict() for m in ms]
    assert lib.hpe_fit_epoch_multi(mixed, 2, 0, _lib.ptr(table), _lib.stream()) == 1
    assert b'kernel instance' in lib.hpe_last_error()
    res = _residual_stack()
    rh = res._eng().program('train', 1).h
    assert lib.hpe_fit_multi_instance(rh) == -1 and lib.hpe_fit_multi_lane_cap(rh) == 0
    torch.cuda.synchronize()
    for m, b in zip(ms, before):
        for k, v in m.weights_dict().items():
            np.testing.assert_array_equal(v, b[k])
    assert lib.hpe_fit_multi_lane_cap(ms[0]._eng().program('train', 1).h) >= ms[0]._eng().fit_groups()


def test_global_seed_state_is_untouched():
    from hpe import random as hrandom
    x, y = features(200, 96, seed=28), labels(200, seed=29)
    specs = [_spec(F=64, seed=3 + i, init_seed=i) for i in range(2)]
    ms = [_compiled(s) for s in specs]
    hpe.set_seed(1234)
    hrandom.generator().standard_normal(3)      # advance the generator: its state must survive too
    state = hrandom.generator().bit_generator.state
    hs = hpe.fit_many(ms, x, y, 128, epochs=1)     # default seeds: hpe.random.seed() + i
    assert hrandom.seed() == 1234
    assert hrandom.generator().bit_generator.state == state
    for i, s in enumerate(specs):
        ref, href = _solo(dict(s, seed=1234 + i), x, y, 1)
        _same(ms[i], hs[i], ref, href, 'trial %d' % i)


def test_one_trial_multi_call_equals_hpe_fit_epoch():
    """The argument packing of the two wrappers: hpe_fit_epoch and hpe_fit_epoch_multi with
    n_trials = 1 run the same solo entry, so two clones of one state (300 rows at batch 128: two
    full batches and a ragged one of 44; Adam with non-zero m / v, dropout 0.2) end byte-equal in
    params, mirror, m, v, the stats rows and the flags word."""
    import torch
    from hpe.engine import OPT_KIND
    lib = _lib.load()
    n, bs, steps = 300, 128, 3
    m = _compiled(_spec(F=64, dropout=0.2))
    eng, opt = m._eng(), m.optimizer
    dev = eng.device
    x, y = features(n, 96, seed=32), labels(n, seed=33)
    xd, yd = torch.from_numpy(x.reshape(n, 96)).to(dev), torch.from_numpy(y).to(dev)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(n).astype(np.int32)).to(dev)
    alpha = torch.from_numpy(eng._alphas_host(opt, steps)).to(dev)
    h = eng.program('train', 1).h
    assert lib.hpe_fit_supported(h, bs) == 1
    st = {'params': eng.params.repeat(2, 1), 'params_t': eng.params_t.repeat(2, 1),
          'm': (torch.rand(eng.n_train, device=dev) * 1e-3).repeat(2, 1),
          'v': (torch.rand(eng.n_train, device=dev) * 1e-6).repeat(2, 1),
          'stats': torch.zeros(2, steps, 2 + 4 * eng.fit_groups(), device=dev),
          'ws': torch.full((2, lib.hpe_fit_workspace_size(h, bs) // 4), 7, dtype=torch.int32, device=dev)}

    def trial(i):
        dp = lambda t: t[i].data_ptr()  # noqa: E731
        return _lib.FitTrial(h.value, dp(st['params']), dp(st['params_t']), dp(st['m']), dp(st['v']),
                             eng.l2.data_ptr(), eng.tpos.data_ptr(), xd.data_ptr(), yd.data_ptr(), perm.data_ptr(),
                             n, bs, OPT_KIND[opt.kind], float(opt.learning_rate), float(opt.beta_1),
                             float(opt.beta_2), float(opt.epsilon), alpha.data_ptr(), 12345, 0,
                             dp(st['stats']), int(st['stats'].shape[2]), dp(st['ws']))

    t = trial(0)
    _lib.check(lib.hpe_fit_epoch(t.prog, t.params, t.params_t, t.m, t.v, t.l2, t.tpos, t.x, t.y_true, t.perm, t.n,
                                 t.batch, t.kind, t.lr, t.beta_1, t.beta_2, t.epsilon, t.alpha, t.seed_base, t.iter0,
                                 t.stats, t.stats_stride, 0, t.workspace, _lib.stream()), 'hpe_fit_epoch')
    table = torch.zeros(lib.hpe_fit_multi_table_size(1), dtype=torch.uint8, device=dev)
    _lib.check(lib.hpe_fit_epoch_multi((_lib.FitTrial * 1)(trial(1)), 1, 0, _lib.ptr(table), _lib.stream()),
               'hpe_fit_epoch_multi')
    torch.cuda.synchronize()
    assert not torch.equal(st['params'][0], eng.params)      # the epoch trained something
    assert (st['stats'][:, :, 0] > 0).all()
    for k in ('params', 'params_t', 'm', 'v', 'stats'):
        got = st[k].cpu().numpy().view(np.uint8).reshape(2, -1)
        assert np.array_equal(got[0], got[1]), k
    ws = st['ws'].cpu().numpy()
    assert ws[0, 1] == ws[1, 1] != 7          # the flags word: zeroed from its 7, then equal
