"""fit_many(residual_stacks=True) against one Model.fit after another: T independent trainings of
create_model_complex(1e-6, 1e-4) (train_88.py's default graph) on one GPU.

Data: BIWI_Train_Enlarged_features_88_0.7_1.npz, 80 / 20 split, batch 128, SGD as train_88.py, a fixed
number of epochs, with and without validation every epoch.  Variant A trains the T models one after
another with Model.fit (hpe_fit_epoch: one workgroup per launch); variant B is one hpe.fit_many
(hpe_res_fit_epoch_multi: T workgroups per launch).  Every T is warmed up first, all runs share one
process, the variants alternate over three rounds, and every timed window ends with a device
synchronise.  Reports trained rows per second per variant (median over the rounds, max - min), and
for B, from one more pass under the library's HIP-event timing (hpe_kernel_timing: the epoch
launches and the validation launches, not the reductions), the epoch launch's device time and the
share of the wall time that is not device time of those kernels ("host share").  Writes every run
to profiles/fit_many_res.json (--out).

  python scripts/fit_many_res_bench.py [--trials 1,8,64,256] [--epochs 300,100,30,20] [--rounds 3] [--out FILE]

--epochs: one count per entry of --trials (or one for all), so that the window of few trials is not a
fraction of a second.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'head-pose-estimation-model_amd')
sys.path.insert(0, PKG)
DATA = os.path.join(ROOT, 'tests', 'golden', 'data', 'BIWI_Train_Enlarged_features_88_0.7_1.npz')


def builder():
    spec = importlib.util.spec_from_file_location('hpe_attention_model_88_bench',
                                                  os.path.join(PKG, 'Model-88', 'attention_model.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.create_model_complex


def models(hpe, keras, make, T):
    out = []
    for s in range(T):
        hpe.set_seed(s)
        keras.backend.clear_session()
        m = make(1e-6, 1e-4)
        m.compile(optimizer=keras.optimizers.SGD(learning_rate=0.00028), loss='mse', metrics=['mae'])
        m._eng().program('train', 1)    # parameters and program on the device before the clock starts
        out.append(m)
    return out


def run(hpe, keras, torch, make, variant, T, data, epochs, val):
    tx, vx, ty, vy = data
    kw = {'validation_data': (vx, vy)} if val else {}
    ms = models(hpe, keras, make, T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if variant == 'A':
        for s, m in enumerate(ms):
            hpe.set_seed(s)
            m.fit(tx, ty, epochs=epochs, batch_size=128, verbose=0, **kw)
    else:
        hpe.fit_many(ms, tx, ty, 128, epochs=epochs, seeds=list(range(T)), residual_stacks=True, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(m._last_fit_fused for m in ms)
    return dt


def timed_pass(hpe, keras, torch, make, lib, check, T, data, epochs, val):
    """One pass of B under hpe_kernel_timing: (wall seconds, ms of every timed launch in order)."""
    cap = epochs * (T + 1) + 16
    check(lib.hpe_kernel_timing(cap), 'hpe_kernel_timing')
    try:
        wall = run(hpe, keras, torch, make, 'B', T, data, epochs, val)
        buf = (ctypes.c_float * cap)()
        k = lib.hpe_kernel_times(buf, cap)
    finally:
        lib.hpe_kernel_timing(0)
    return wall, np.array(buf[:max(k, 0)], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', default='300,100,30,20')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trials', default='1,8,64,256')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_many_res.json'))
    a = ap.parse_args()
    import torch
    import hpe
    from hpe import _lib, keras
    from hpe.data import train_test_split
    lib = _lib.load()
    make = builder()
    d = np.load(DATA)
    data = train_test_split(d['features'].reshape(-1, 1, 1, 88).astype(np.float32), d['poses'].reshape(-1, 1, 1, 3),
                            test_size=0.2, random_state=42)
    n = len(data[0])
    Ts = [int(t) for t in a.trials.split(',')]
    eps = [int(e) for e in a.epochs.split(',')]
    eps = eps * len(Ts) if len(eps) == 1 else eps
    if len(eps) != len(Ts):
        ap.error('--epochs needs one count, or one per entry of --trials')
    out = {'what': 'T trainings of create_model_complex(1e-6, 1e-4), SGD, batch 128: A = one Model.fit after '
                   'another, B = one hpe.fit_many(residual_stacks=True); wall seconds, device synchronised',
           'rounds': a.rounds, 'train_rows': n, 'val_rows': len(data[1]), 'results': []}
    for val in (True, False):
        for T, epochs in zip(Ts, eps):
            for v in 'AB':                                 # warm-up of every shape and variant
                run(hpe, keras, torch, make, v, T, data, 2, val)
            sec = {'A': [], 'B': []}
            for _ in range(a.rounds):                      # alternate the variants
                for v in 'AB':
                    sec[v].append(run(hpe, keras, torch, make, v, T, data, epochs, val))
            rows = {v: [T * n * epochs / s for s in sec[v]] for v in 'AB'}
            wall, ms = timed_pass(hpe, keras, torch, make, lib, _lib.check, T, data, epochs, val)
            # per epoch: the epoch launch, then T validation launches (left out if the count says otherwise)
            per = T + 1 if val else 1
            epoch_ms = ms[::per] if ms.size == epochs * per else ms[:0]
            r = {'T': T, 'validation': val, 'epochs': epochs, 'A_seconds': sec['A'], 'B_seconds': sec['B'],
                 'A_rows_per_s_median': float(np.median(rows['A'])), 'A_rows_per_s_spread': max(rows['A']) - min(rows['A']),
                 'B_rows_per_s_median': float(np.median(rows['B'])), 'B_rows_per_s_spread': max(rows['B']) - min(rows['B']),
                 'B_over_A': float(np.median(rows['B']) / np.median(rows['A'])),
                 'launches_per_epoch': len(hpe.fit_many.last_plan['launches'][-1]),
                 'timed_pass': {'wall_seconds': wall, 'timed_launches': int(ms.size),
                                'epoch_launch_ms_median': float(np.median(epoch_ms)) if epoch_ms.size else None,
                                'device_ms_total': float(ms.sum()),
                                'host_share': float(1.0 - ms.sum() * 1e-3 / wall)}}
            out['results'].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
