"""Seed spread of a from-scratch Model-96 training run (PARITY UNPINNED).

Trains create_model(num_filters=360, dropout 0, l2 0.05) — the sqnu665j hyper-parameters (its
model_config: Conv2D(360, tanh, L2 0.05) -> SpatialDropout2D(0) -> Conv2D(3, L2 0.05)) — with
train_96.py's own loop (Model-96/train_96.py:42-57 config, :142-183 split / callbacks / fit): legacy
Adam lr 2.8e-4, batch 128, 80/20 train_test_split(random_state=42), EarlyStopping(val_loss,
patience 40, min_delta 1e-3, restore_best_weights), then evaluate on AFLW2000_features_96 and
BIWI_Test_Enlarged_features_96.  One run per seed (weight init + shuffles), all on this GPU through
Model.fit (fused epoch launches), one after another; with --together all seeds train side by side
through hpe.fit_many (several per epoch launch, the same results per seed).

The reference's training set BIWI_train_features_96.npz is a missing blob in the reference
checkout, so the substitute is BIWI_Train_Enlarged_features_96_0.7_1.npz (1,643 rows).  The result
is a distribution to set beside sqnu665j's AFLW2000 MAE of 7.7826, not a parity
claim.  Writes gpurun_out/seed_spread_96.json.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
DATA = os.path.join(ROOT, 'tests', 'golden', 'data')


def create_model(keras, F=360, l2=0.05, dropout=0.0):
    reg = keras.regularizers.l2(l2)
    inp = keras.Input(shape=(None, None, 96))
    x = keras.layers.Conv2D(F, 1, padding='same', activation='tanh', bias_regularizer=reg, kernel_regularizer=reg)(inp)
    x = keras.layers.SpatialDropout2D(dropout)(x)
    o = keras.layers.Conv2D(3, 1, padding='same', bias_regularizer=reg, kernel_regularizer=reg)(x)
    o = keras.layers.SpatialDropout2D(dropout)(o)
    m = keras.Model(inp, o)
    m.compile(optimizer=keras.optimizers.Adam(learning_rate=0.00028), loss='mse', metrics=['mae'])
    return m


def load(name):
    d = np.load(os.path.join(DATA, name))
    return d['features'].reshape(-1, 1, 1, 96).astype(np.float32), d['poses'].reshape(-1, 1, 1, 3)


def main(seeds, max_epochs, together=False):
    import hpe
    from hpe import keras
    from hpe.data import train_test_split
    x, y = load('BIWI_Train_Enlarged_features_96_0.7_1.npz')
    tx, vx, ty, vy = train_test_split(x, y, test_size=0.2, random_state=42)
    ax, ay = load('AFLW2000_features_96_0.7_1.npz')
    bx, by = load('BIWI_Test_Enlarged_features_96_0.7_1.npz')
    runs = []
    os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
    def early_stop():
        return keras.callbacks.EarlyStopping(monitor='val_loss', patience=40, min_delta=0.001,
                                             restore_best_weights=True)

    ms, hs = [], []
    if together:    # every seed's model initialised under its own seed, then one fit_many
        for s in seeds:
            hpe.set_seed(s)
            keras.backend.clear_session()
            ms.append(create_model(keras))
        t0 = time.perf_counter()
        hs = hpe.fit_many(ms, tx, ty, 128, epochs=max_epochs, seeds=seeds, validation_data=(vx, vy),
                          callbacks=[[early_stop()] for _ in seeds])
        dts = [(time.perf_counter() - t0) / len(seeds)] * len(seeds)   # the call's time, shared equally
    for i, s in enumerate(seeds):
        if together:
            m, h, dt = ms[i], hs[i], dts[i]
        else:
            hpe.set_seed(s)
            keras.backend.clear_session()
            m = create_model(keras)
            t0 = time.perf_counter()
            h = m.fit(tx, ty, epochs=max_epochs, batch_size=128, validation_data=(vx, vy), callbacks=[early_stop()],
                      verbose=0)
            dt = time.perf_counter() - t0
        _, a_mae = m.evaluate(ax, ay, verbose=0)
        _, b_mae = m.evaluate(bx, by, verbose=0)
        pa = m.predict(ax).reshape(-1, 3)
        per = np.mean(np.abs(pa - ay.reshape(-1, 3)), axis=0)
        r = {'seed': s, 'epochs': len(h.history['loss']), 'best_epoch': int(np.argmin(h.history['val_loss'])) + 1,
             'best_val_loss': float(np.min(h.history['val_loss'])), 'aflw2000_mae': float(a_mae),
             'aflw2000_mae_yaw_pitch_roll': [float(v) for v in per], 'biwi_test_enlarged_mae': float(b_mae),
             'fit_seconds': dt, 'fused_epochs': bool(getattr(m, '_last_fit_fused', False))}
        runs.append(r)
        print(json.dumps(r), flush=True)
    a = np.array([r['aflw2000_mae'] for r in runs])
    out = {'what': 'create_model(360, dropout 0, l2 0.05) trained from scratch per seed on '
                   'BIWI_Train_Enlarged_features_96 (substitute for the missing BIWI_train_features_96), '
                   'train_96.py loop; AFLW2000 MAE vs sqnu665j 7.7826 -- parity unpinned',
           'reference_sqnu665j_aflw2000_mae': 7.7826, 'runs': runs,
           'aflw2000_mae_mean': float(a.mean()), 'aflw2000_mae_std': float(a.std(ddof=1)) if len(a) > 1 else 0.0,
           'aflw2000_mae_min': float(a.min()), 'aflw2000_mae_max': float(a.max())}
    with open(os.path.join(ROOT, 'gpurun_out', 'seed_spread_96.json'), 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != 'runs'}), flush=True)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--together']
    n = int(args[0]) if args else 8
    main(list(range(n)), int(args[1]) if len(args) > 1 else 10000, together='--together' in sys.argv[1:])
