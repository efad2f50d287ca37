"""fit_many against one Model.fit after another: T independent trainings on one GPU.

Shapes: create_model(360, l2 0.05) on BIWI_Train_Enlarged_features_96 (1,314 / 329 split) and
create_model(64) on the 88-channel set, batch 128, validation every epoch, a fixed number of epochs
(300), no early stopping.  Variant A trains the T models one after another with Model.fit (the
solo epoch launch); variant B is one hpe.fit_many.  Every shape is warmed up first, all runs share
one process, the variants alternate over three rounds, and every timed window ends with a device
synchronise.  Reports wall seconds per variant and round, trained rows per second, B / A per T and
the spread of A over its rounds; writes profiles/fit_many.json (--out).

  python scripts/fit_many_bench.py [--epochs 300] [--rounds 3] [--trials 1,2,4,8,16] [--out FILE]
  python scripts/fit_many_bench.py --trace-only      # T = 8, a few epochs of B: for a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
DATA = os.path.join(ROOT, 'tests', 'golden', 'data')

SHAPES = {'96x360': ('BIWI_Train_Enlarged_features_96_0.7_1.npz', 96, 360),
          '88x64': ('BIWI_Train_Enlarged_features_88_0.7_1.npz', 88, 64)}


def create_model(keras, cin, F, l2=0.05):
    reg = keras.regularizers.l2(l2)
    inp = keras.Input(shape=(None, None, cin))
    x = keras.layers.Conv2D(F, 1, padding='same', activation='tanh', bias_regularizer=reg, kernel_regularizer=reg)(inp)
    x = keras.layers.SpatialDropout2D(0.0)(x)
    o = keras.layers.Conv2D(3, 1, padding='same', bias_regularizer=reg, kernel_regularizer=reg)(x)
    o = keras.layers.SpatialDropout2D(0.0)(o)
    m = keras.Model(inp, o)
    m.compile(optimizer=keras.optimizers.Adam(learning_rate=0.00028), loss='mse', metrics=['mae'])
    return m


def load(name, cin):
    d = np.load(os.path.join(DATA, name))
    return d['features'].reshape(-1, 1, 1, cin).astype(np.float32), d['poses'].reshape(-1, 1, 1, 3)


def models(hpe, keras, cin, F, T):
    out = []
    for s in range(T):
        hpe.set_seed(s)
        keras.backend.clear_session()
        m = create_model(keras, cin, F)
        m._eng()        # parameters on the device before the clock starts
        out.append(m)
    return out


def run(hpe, keras, torch, variant, cin, F, T, data, epochs):
    tx, vx, ty, vy = data
    ms = models(hpe, keras, cin, F, T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if variant == 'A':
        for s, m in enumerate(ms):
            hpe.set_seed(s)
            m.fit(tx, ty, epochs=epochs, batch_size=128, validation_data=(vx, vy), verbose=0)
            assert m._last_fit_fused
    else:
        hpe.fit_many(ms, tx, ty, 128, epochs=epochs, seeds=list(range(T)), validation_data=(vx, vy))
        assert all(m._last_fit_fused for m in ms)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trials', default='1,2,4,8,16')
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_many.json'))
    a = ap.parse_args()
    import torch
    import hpe
    from hpe import keras
    from hpe.data import train_test_split
    if a.trace_only:
        name, cin, F = SHAPES['96x360']
        data = train_test_split(*load(name, cin), test_size=0.2, random_state=42)
        run(hpe, keras, torch, 'B', cin, F, 8, data, 2)     # warm-up
        print(json.dumps({'trace_only': True, 'T': 8, 'epochs': 5,
                          'seconds': run(hpe, keras, torch, 'B', cin, F, 8, data, 5)}))
        return
    Ts = [int(t) for t in a.trials.split(',')]
    out = {'what': 'T trainings of create_model(F) at batch 128, %d epochs, validation every epoch: A = one '
                   'Model.fit after another, B = one hpe.fit_many; wall seconds, device synchronised' % a.epochs,
           'epochs': a.epochs, 'rounds': a.rounds, 'shapes': {}}
    for key, (name, cin, F) in SHAPES.items():
        data = train_test_split(*load(name, cin), test_size=0.2, random_state=42)
        n = len(data[0])
        for T in Ts:                                       # warm-up of every shape and variant
            for v in 'AB':
                run(hpe, keras, torch, v, cin, F, T, data, 3)
        rows = []
        for T in Ts:
            sec = {'A': [], 'B': []}
            for _ in range(a.rounds):                      # alternate the variants
                for v in 'AB':
                    sec[v].append(run(hpe, keras, torch, v, cin, F, T, data, a.epochs))
            ma, mb = float(np.median(sec['A'])), float(np.median(sec['B']))
            r = {'T': T, 'A_seconds': sec['A'], 'B_seconds': sec['B'],
                 'A_rows_per_s': T * n * a.epochs / ma, 'B_rows_per_s': T * n * a.epochs / mb,
                 'A_over_B': ma / mb, 'A_spread': (max(sec['A']) - min(sec['A'])) / ma,
                 'launches_per_epoch': len(hpe.fit_many.last_plan['launches'][-1])}
            rows.append(r)
            print(json.dumps(dict(r, shape=key)), flush=True)
        out['shapes'][key] = {'train_rows': n, 'val_rows': len(data[1]), 'F': F, 'cin': cin, 'results': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
