"""The whole-epoch launch's one host driver (run_epochs), and fit_many: train independent models
("trials") side by side, several per epoch launch.

Model.fit's fused path is the driver with one trial, fit_many the driver with several: the epoch
launch, the flag decoding, the exact re-run, the timeout rollback, the read-back and the callback
loop exist once, so "model i ends bit-identical to its solo fit" is one code path, not two kept in
step.  A launch of one trial runs the kernels' solo entry (hpe_fit_epoch_multi and
hpe_res_fit_epoch_multi with n_trials = 1), of several the multi entry.

The whole-epoch kernel of the reference's regime (csrc/hpe_fit.hip: 1x1 maps, the create_model
family, batch <= 512) uses one workgroup per 32 hidden units in one eighth of its grid.
hpe_fit_epoch_multi fills the rest of the grid with further trials, each a closed group of
workgroups running exactly the arithmetic of a solo launch, so every model ends bit-identical to

    hpe.set_seed(seeds[i]); models[i].fit(x, y, batch_size=..., epochs=..., ...)

on the fused path.  Per epoch the host groups the active trials by kernel instance, splits each group
into launches (hpe_fit_multi_plan), uploads all permutations and step sizes in one transfer and
reads every trial's flags, statistics and validation sums back in one.

Residual stacks (create_model_complex and the stacks like it, csrc/hpe_res.hip) train with one
workgroup for the whole epoch; with residual_stacks=True they are trials too, block b of one
hpe_res_fit_epoch_multi launch per kernel instance training trial b, beside the create_model-family
launches of the same call.
"""
import ctypes
import math
import os
import warnings

import numpy as np

from . import _lib
from . import random as hrandom
from .callbacks import History
from .model import epoch_logs

_MASK = 0xFFFFFFFFFFFFFFFF


class _Trial:
    """One model of an epoch launch.  label prefixes its verbose line, timeout opens its warning
    when the workgroup exchange times out: the caller's texts (Model.fit's or fit_many's)."""

    def __init__(self, i, model, bs, seed, callbacks, n, label, timeout):
        self.i, self.model, self.bs, self.seed = i, model, bs, int(seed)
        self.label, self.timeout = label, timeout
        self.eng = model._eng()
        self.res = self.eng.program('train', 1).prog.kind == 'res'   # one workgroup per trial, never flags
        self.steps = math.ceil(n / bs)
        self.nbs = [min(n, (s + 1) * bs) - s * bs for s in range(self.steps)]
        self.rng = np.random.RandomState(self.seed)       # Model.fit's shuffle stream
        self.seed_base = (self.seed * 1000003) & _MASK    # hpe.random.dropout_seed(0) under this seed
        self.hist = History()
        self.cbs = [self.hist] + list(callbacks or [])
        self.fused = True
        self.active = True
        self.stats = None     # device [steps, 2 + 4 G] (fused) or [steps, 2 + optimizer grid]
        self.saved = None


def _refuse(i, why):
    raise ValueError('fit_many: model %d: %s' % (i, why))


def _check(models, batch_sizes, C, P, residual_stacks=False):
    """Everything fit_many refuses, before any model is trained."""
    env = os.environ.get('HPE_FIT_FUSED')
    for i, (m, bs) in enumerate(zip(models, batch_sizes)):
        if getattr(m, 'optimizer', None) is None:
            _refuse(i, 'is not compiled (model.compile(optimizer, loss))')
        if m._dist is not None:
            _refuse(i, 'is data-parallel (distribute()); fit_many trains on one GPU')
        if env == '0':
            _refuse(i, 'HPE_FIT_FUSED=0 forces the per-step path; fit_many is the fused path')
        if P != 1:
            _refuse(i, 'the epoch launch trains on 1x1 maps, got %d pixels per image' % P)
        cin = m._config['layers'][0]['config']['batch_input_shape'][-1]
        if cin != C:
            _refuse(i, 'expects %d input channels, x has %d' % (cin, C))
    lib = _lib.load()
    for i, (m, bs) in enumerate(zip(models, batch_sizes)):
        eng = m._eng()
        c = eng.program('train', 1)
        res = c.prog.kind == 'res'
        if res and not residual_stacks:
            _refuse(i, 'residual-stack programs run one per launch (Model.fit)')
        if bs > eng.FIT_FUSED_AUTO_MAX and env != '1':
            _refuse(i, 'batch %d is above %d: set HPE_FIT_FUSED=1 to train it on the fused path'
                    % (bs, eng.FIT_FUSED_AUTO_MAX))
        if getattr(eng, '_fit_disabled', False):
            _refuse(i, 'an earlier epoch launch of this model timed out (fused path disabled)')
        inst = lib.hpe_res_fit_multi_instance(c.h) if res else lib.hpe_fit_multi_instance(c.h)
        if c.prog.kind not in ('mlp2', 'res') or lib.hpe_fit_supported(c.h, int(bs)) != 1 or inst < 0:
            _refuse(i, 'the epoch launch does not support this program at batch %d (hpe_fit_supported)' % bs)


def plan_launches(groups, lane_cap):
    """Split trials of `groups[i]` workgroups (one kernel instance) into launches with
    hpe_fit_multi_plan: a list of index lists, in input order."""
    lib = _lib.load()
    out, rest = [], list(range(len(groups)))
    while rest:
        g = (ctypes.c_int32 * len(rest))(*[groups[i] for i in rest])
        lane = (ctypes.c_int32 * len(rest))()
        first = (ctypes.c_int32 * len(rest))()
        k = lib.hpe_fit_multi_plan(g, len(rest), int(lane_cap), lane, first)
        if k < 1:
            raise _lib.HPEError('hpe_fit_multi_plan placed none of %d trials (lane cap %d)' % (len(rest), lane_cap))
        out.append(rest[:k])
        rest = rest[k:]
    return out


def _launch(trials, exact, tables, record):
    """One epoch of `trials` (fused): grouped by kernel instance, split into launches.  The
    create_model family goes through hpe_fit_multi_plan and hpe_fit_epoch_multi; residual stacks
    need no plan (a trial is one workgroup that waits for no other): one hpe_res_fit_epoch_multi
    launch per instance, whatever the number of trials."""
    import torch
    lib = _lib.load()

    def table(need, dev):
        slot = len(record)
        if slot >= len(tables) or tables[slot].numel() < need:
            tables[slot:slot + 1] = [torch.empty(need, dtype=torch.uint8, device=dev)]
        return _lib.ptr(tables[slot])

    by_inst = {}
    for t in trials:
        h = t.eng.program('train', 1).h
        key = (1, lib.hpe_res_fit_multi_instance(h)) if t.res else (0, lib.hpe_fit_multi_instance(h))
        by_inst.setdefault(key, []).append(t)
    for res, inst in sorted(by_inst):
        ts = by_inst[res, inst]
        dev = ts[0].eng.device
        if res:
            arr = (_lib.FitTrial * len(ts))(*[t.ft for t in ts])
            tab = table(lib.hpe_res_fit_multi_table_size(len(ts)), dev)
            _lib.check(lib.hpe_res_fit_epoch_multi(arr, len(ts), tab, _lib.stream()), 'hpe_res_fit_epoch_multi')
            record.append([t.i for t in ts])
            continue
        split = [[0]]   # one trial runs the kernel's solo entry (hpe_fit_supported): nothing to place
        if len(ts) > 1:
            cap = lib.hpe_fit_multi_lane_cap(ts[0].eng.program('train', 1).h)
            split = plan_launches([t.eng.fit_groups() for t in ts], cap)
        for idxs in split:
            arr = (_lib.FitTrial * len(idxs))(*[ts[j].ft for j in idxs])
            tab = table(lib.hpe_fit_multi_table_size(len(idxs)), dev)
            _lib.check(lib.hpe_fit_epoch_multi(arr, len(idxs), int(exact), tab, _lib.stream()), 'hpe_fit_epoch_multi')
            record.append([ts[j].i for j in idxs])


def fit_many(models, x, y, batch_size, epochs=1, seeds=None, validation_data=None, callbacks=None,
             shuffle=True, initial_epoch=0, verbose=0, residual_stacks=False):
    """Train `models` (compiled hpe.Models, each with its own weights, optimizer, dropout and L2;
    widths may differ) on the shared x / y, several per epoch launch.  batch_size: an int or one per
    model; seeds: one per model (default hpe.random.seed() + i); callbacks: None or one list per
    model.  Returns one History per model; model i ends exactly as after hpe.set_seed(seeds[i]) and
    models[i].fit(...) alone on the fused path.  The global seed state is left as it was.
    residual_stacks=True also accepts residual-stack models (create_model_complex and the stacks
    like it): each is one workgroup of an hpe_res_fit_epoch_multi launch, one launch per kernel
    instance, and a call may mix them with the create_model family.  The default stays False, which
    refuses them by name as before this keyword existed: that refusal is part of the tested
    behaviour, and making True the default is a change of its own.
    fit_many.last_plan records, per epoch, the launches made (lists of model indices), every
    trial's flags word and the trials re-run on the exact-fp32 path."""
    import torch
    models = list(models)
    T = len(models)
    if T == 0:
        return []
    bss = [int(batch_size)] * T if np.isscalar(batch_size) else [int(b) for b in batch_size]
    seeds = [hrandom.seed() + i for i in range(T)] if seeds is None else [int(s) for s in seeds]
    callbacks = [None] * T if callbacks is None else list(callbacks)
    if not (len(bss) == len(seeds) == len(callbacks) == T):
        raise ValueError('fit_many: batch_size, seeds and callbacks need one entry per model (%d)' % T)
    rows, n, P, _ = models[0]._rows(x)
    lab = models[0]._labels(y, n)
    _check(models, bss, rows.shape[1], P, residual_stacks)
    if validation_data is not None:
        vrows, vn, vP, _ = models[0]._rows(validation_data[0])
        vlab = models[0]._labels(validation_data[1], vn)
        if vrows.shape[1] != rows.shape[1] or vP != 1:
            raise ValueError('fit_many: validation_data must have x\'s channels on 1x1 maps')
    dev = models[0]._eng().device
    xd, yd = torch.from_numpy(rows).to(dev), torch.from_numpy(lab).to(dev)
    val = None
    if validation_data is not None:
        val = (torch.from_numpy(vrows).to(dev), torch.from_numpy(vlab).to(dev), vn)
    trials = [_Trial(i, m, bss[i], seeds[i], callbacks[i], n, 'Model %d - ' % i,
                     'hpe_fit_epoch_multi: workgroup exchange of model %d timed out' % i)
              for i, m in enumerate(models)]
    pool = begin(trials, epochs, verbose)
    fit_many.last_plan = {'launches': [], 'flags': [], 'exact': []}
    return run_epochs(trials, pool, xd, yd, val, n, epochs, initial_epoch, shuffle, verbose, fit_many.last_plan)


fit_many.last_plan = None


def begin(trials, epochs, verbose):
    """Start training `trials`: every trial's fused stats rows [steps, 2 + 4 G] as slices of one pool
    (one zero fill and one slice of the read-back per epoch), which is returned, and the callbacks'
    train-begin calls."""
    import torch
    offs = np.cumsum([0] + [t.steps * (2 + 4 * t.eng.fit_groups()) for t in trials])
    pool = torch.zeros(int(offs[-1]), dtype=torch.float32, device=trials[0].eng.device)
    for k, t in enumerate(trials):
        t.stats = pool[int(offs[k]):int(offs[k + 1])].view(t.steps, -1)
        t.model._last_fit_fused = True
        for cb in t.cbs:
            cb.set_model(t.model)
            cb.set_params({'epochs': epochs, 'steps': t.steps, 'verbose': verbose})
        t.model.stop_training = False
        for cb in t.cbs:
            cb.on_train_begin()
    return pool


def run_epochs(trials, pool, xd, yd, valid, n, epochs, initial_epoch, shuffle, verbose, plan):
    """The one driver of the whole-epoch launch, for Model.fit (one trial) and fit_many alike: per
    epoch, one upload of every active trial's permutation and step sizes, the launches, one read-back
    of flags, stats and validation sums, the exact re-run of trials whose fp16 range was exceeded, the
    rollback of trials whose workgroup exchange timed out (fused path disabled for that engine, this
    and later epochs through Engine.fit_steps), then logs and callbacks.  trials and pool: from
    begin(); xd / yd: the n device rows and labels; valid: None, or (rows, labels, image count) of the
    validation set; plan: None, or the dict that records each epoch's launches, flags words and
    exact re-runs.  Returns the Histories."""
    import torch
    dev = xd.device
    vxd, vyd, vn = valid or (None, None, 0)
    vP = vxd.shape[0] // vn if vn else 1
    tables = []

    def per_step(t, idx):   # the per-step epoch of a trial whose fused path is disabled
        t.eng.fit_steps(t.model.optimizer, xd, yd, idx, t.bs, t.stats, t.seed_base, 0.0, 1)

    def validate(t):
        if valid is None:
            return []
        e = t.eng
        return [e.loss_sums(vxd, vyd, vP), (e.l2 * e.params[:e.n_train] ** 2).sum().reshape(1)]

    for epoch in range(initial_epoch, epochs):
        act = [t for t in trials if t.active]
        if not act:
            break
        for t in act:
            for cb in t.cbs:
                cb.on_epoch_begin(epoch)
        # all permutations and optimizer step sizes in one upload
        perms = [(t.rng.permutation(n) if shuffle else np.arange(n)).astype(np.int32) for t in act]
        alphas = [t.eng._alphas_host(t.model.optimizer, t.steps).view(np.int32) for t in act]
        blob = torch.from_numpy(np.concatenate(perms + alphas)).to(dev)
        o = n * len(act)
        for k, t in enumerate(act):
            t.idx = blob[k * n:(k + 1) * n]
            t.alpha = blob[o:o + t.steps].view(torch.float32)
            o += t.steps
        pool.zero_()
        fused = [t for t in act if t.fused]
        for t in fused:
            t.ft = t.eng.fit_trial(t.model.optimizer, xd, yd, t.idx, t.bs, t.stats, t.seed_base, t.alpha)
            # what a flagged epoch restores; a residual stack never flags (exact fp32, no exchange)
            t.saved = None if t.res else [s.clone() for s in t.eng.fit_state()]
        record = []
        _launch(fused, 0, tables, record)
        for t in act:
            if not t.fused:
                per_step(t, t.idx)

        def read_back(ts):   # flags, stats and validation sums of `ts` in one device-to-host copy
            parts, cuts = [], []
            for t in ts:
                p = ([t.eng.fit_flag_word()] if t.fused else []) + [t.stats.reshape(-1).view(torch.int32)] + \
                    [v.view(torch.int32) for v in validate(t)]
                parts += p
                cuts.append([q.numel() for q in p])
            host = torch.cat(parts).cpu().numpy()
            out, o = {}, 0
            for t, cut in zip(ts, cuts):
                f = []
                for c in cut:
                    f.append(host[o:o + c])
                    o += c
                flag = int(f.pop(0)[0]) if t.fused else 0
                st = f[0].view(np.float32).reshape(t.steps, -1)
                val = (f[1].view(np.float32), vn * vP * 3, float(f[2].view(np.float32)[0])) if len(f) > 1 else None
                out[t.i] = (flag, st, val)
            return out

        res = read_back(act)
        flags = {t.i: res[t.i][0] for t in act}
        for t in fused:
            assert not (t.res and flags[t.i]), 'residual-stack trial %d set flags %d' % (t.i, flags[t.i])
        redo = [t for t in fused if res[t.i][0]]
        exact = [t for t in redo if res[t.i][0] & 1 and not res[t.i][0] & 2]
        if exact:   # fp16 range exceeded: these trials redo the epoch exactly, together
            for t in exact:
                t.eng._restore(t.saved)
                t.stats.zero_()
            _launch(exact, 1, tables, record)
            again = read_back(exact)
            res.update(again)
            for t in exact:
                flags[t.i] |= again[t.i][0]
        timed = [t for t in redo if res[t.i][0] & 2]
        if timed:   # roll back, disable the fused path, this and later epochs per step
            for t in timed:
                t.eng._restore(t.saved)
                t.eng._fit_disabled = True
                t.fused = t.model._last_fit_fused = False
                warnings.warn(t.timeout + '; epoch re-run on the per-step path')
                t.stats = torch.zeros((t.steps, 2 + t.eng.optim_grid()), dtype=torch.float32, device=dev)
                per_step(t, t.idx)
            res.update(read_back(timed))
        if plan is not None:
            plan['launches'].append(record)
            plan['flags'].append([flags.get(t.i, 0) for t in trials])
            plan['exact'].append([t.i for t in exact])
        for t in act:
            if t.fused:
                t.eng.iterations += t.steps
            t.saved = None
            _, st, val = res[t.i]
            logs = epoch_logs(st, t.nbs, n, 1, val)
            t.model.optimizer.iterations = t.eng.iterations
            if verbose and verbose != 0:
                print(t.label + 'Epoch %d/%d - ' % (epoch + 1, epochs) +
                      ' - '.join('%s: %.4f' % (k, v) for k, v in logs.items()))
            for cb in t.cbs:
                cb.on_epoch_end(epoch, logs)
            if t.model.stop_training:
                t.active = False
                _end(t)
    for t in trials:
        if t.active:
            _end(t)
    return [t.hist for t in trials]


def _end(t):
    t.active = False
    for cb in t.cbs:
        cb.on_train_end()
    t.model.history = t.hist
    t.hist.model = t.model
