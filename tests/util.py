"""Shared helpers for the parity tests (fixtures, synthetic inputs, oracle glue)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODELS = os.path.join(GOLDEN, 'models')
DATA = os.path.join(GOLDEN, 'data')

# forward tolerance: the reference's own rtol (InputShapeConvertor.py:205) with
# atol widened to 1e-4 degrees for accumulation-order differences
RTOL, ATOL = 1e-5, 1e-4


def index():
    with open(os.path.join(MODELS, 'index.json')) as fh:
        return json.load(fh)['models']


def fixture(rid):
    with open(os.path.join(MODELS, rid + '.json')) as fh:
        meta = json.load(fh)
    w = dict(np.load(os.path.join(MODELS, rid + '.npz')))
    return meta['model_config'], w


def input_channels(mc):
    return mc['config']['layers'][0]['config']['batch_input_shape'][-1]


def features(n, c, seed=0, h=1, w=1):
    """Synthetic post-ReLU-like BlazeFace features: max(0, 0.6 N(0,1) - 0.3)."""
    rng = np.random.default_rng(seed)
    return np.maximum(0.0, 0.6 * rng.standard_normal((n, h, w, c)) - 0.3).astype(np.float32)


def labels(n, seed=1):
    return (20.0 * np.random.default_rng(seed).standard_normal((n, 3))).astype(np.float32)


def oracle_step(mc, w, x, y, layout, seed, image_offset=0, dtype=None):
    """One training forward + autograd of the data term (mse) by the oracle, float64 unless dtype
    says otherwise, with the dropout masks of (seed, image_offset).  Returns (gradient in the
    engine's flat parameter order as float64, sum e^2, sum |e|)."""
    import torch
    from oracle import keras_ref as K
    g = K.Graph(mc, w) if dtype is None else K.Graph(mc, w, dtype=dtype)
    tr = list(g.trainable)
    for k in tr:
        g.params[k].requires_grad_(True)
    p = g.forward(x, training=True, drop_seed=seed, image_offset=image_offset)
    yt = torch.tensor(np.asarray(y), dtype=g.dtype)
    yb = yt.reshape(yt.shape[0], *([1] * (p.dim() - 2)), 3).expand_as(p)
    gr = torch.autograd.grad(K.mse(yb, p), [g.params[k] for k in tr])
    flat = np.zeros(sum(int(np.prod(s)) for _, s in layout.param_index.values()))
    for k, gk in zip(tr, gr):
        o, shp = layout.param_index[k]
        flat[o:o + int(np.prod(shp))] = gk.detach().numpy().ravel()
    e = (p - yb).detach().double()
    return flat, float((e * e).sum()), float(e.abs().sum())


def data_grad64(mc, w, x, y, layout, seed, image_offset=0):
    """float64 oracle gradient of the data term (mse) in the engine's flat parameter order."""
    return oracle_step(mc, w, x, y, layout, seed, image_offset)[0]


def check_gradient(tag, mc, w, eng, g, x, y, seed, img_off=0):
    """The kernel's gradient g (n_train + 4 words; eng: its Engine) against the float64 oracle on
    (x, y) in batch order with the dropout masks of (seed, img_off): whole-gradient bar 1e-5, every
    parameter tensor normwise over itself within max(1e-5, 4 x the fp32 oracle's error), a tensor
    whose float64 gradient is zero exactly zero, both loss sums at rtol 1e-5.  Returns the worst
    tensor's (kernel error, fp32-oracle error, name)."""
    import time
    import torch
    t0 = time.time()
    g64, sse, sae = oracle_step(mc, w, x, y, eng.layout, seed, image_offset=img_off)
    g32 = oracle_step(mc, w, x, y, eng.layout, seed, image_offset=img_off, dtype=torch.float32)[0]
    npt = eng.n_train
    assert g.shape[0] == npt + 4 and g64.shape[0] == npt
    assert np.isfinite(g).all()
    err = np.abs(g[:npt] - g64).max() / np.abs(g64).max()
    worst = (0.0, 0.0, '')
    fails = []
    for k, (o, shp) in eng.layout.param_index.items():
        sl = slice(o, o + int(np.prod(shp)))
        scale = np.abs(g64[sl]).max()
        if scale == 0.0:
            if np.any(g[sl] != 0.0):
                fails.append((k, 'float64 gradient is zero, kernel max |g| = %.2e' % np.abs(g[sl]).max()))
            continue
        ek = np.abs(g[sl] - g64[sl]).max() / scale
        e32 = np.abs(g32[sl] - g64[sl]).max() / scale
        if ek > worst[0]:
            worst = (ek, e32, k)
        if ek > max(1e-5, 4 * e32):
            fails.append((k, 'kernel %.2e, fp32 oracle %.2e' % (ek, e32)))
    print('%s: max |g - g64| / max |g64| = %.2e; worst tensor %s: kernel %.2e, fp32 oracle %.2e (oracle %.1f s)'
          % (tag, err, worst[2], worst[0], worst[1], time.time() - t0))
    assert err <= 1e-5, err
    assert not fails, fails
    np.testing.assert_allclose(g[npt], sse, rtol=1e-5)
    np.testing.assert_allclose(g[npt + 1], sae, rtol=1e-5)
    return worst
