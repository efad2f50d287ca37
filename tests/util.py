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
