"""Small synthetic graphs for the generic row-program tests — TEST INFRASTRUCTURE, not a test.

Builders over hpe.keras that return (model_config, weights) with seeded weights.  Every graph has
96 or 88 input channels and 3 outputs, and each is shaped to reach one part of the generic
training path (csrc/hpe_rowprog.hip) that the reference's checkpoints reach rarely or never: pad
channels under activations with act(0) != 0, stand-alone Activation layers, gradient accumulation
into a shared tensor, thin (N <= 8) layers, LayerNormalization at P > 1, the SE / MHA gate,
SeparableConv2D, and the two large-program geometries (several passes, slots in device scratch).

Weights are drawn, not Glorot-initialised: a first-layer kernel has unit variance, so that on
util.features (rms 0.27 over 88 / 96 channels) the pre-activations have a standard deviation of
about 2.6 and both signs; later kernels have std 2 / sqrt(fan_in); biases, beta and the offsets of
gamma / depthwise kernels are N(0, 0.3).
"""
import numpy as np

from hpe import keras
from hpe.layers import _ACTIVATIONS
from util import fixture

ACTIVATIONS = tuple(_ACTIVATIONS)
kl = keras.layers


def _seeded(model, seed):
    """(model_config, weights) of a built model with every weight redrawn from `seed`."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, a in model.weights_dict().items():
        base = k.rsplit('/', 1)[-1]
        if base in ('kernel', 'pointwise_kernel'):
            if k.endswith('attention_output/kernel'):
                fan_in = a.shape[0] * a.shape[1]
            elif a.ndim == 4:
                fan_in = a.shape[2]
            else:
                fan_in = a.shape[0]
            std = 1.0 if fan_in in (88, 96) else 2.0 / np.sqrt(fan_in)
            v = std * rng.standard_normal(a.shape)
        elif base in ('gamma', 'depthwise_kernel'):
            v = 1.0 + 0.3 * rng.standard_normal(a.shape)
        else:   # bias, beta
            v = 0.3 * rng.standard_normal(a.shape)
        w[k] = v.astype(np.float32)
    return model.model_config, w


def _input(cin):
    keras.backend.clear_session()
    return keras.Input(shape=(None, None, cin))


def act_chain(act, cin=96, seed=1, widths=(40, 24)):
    """in -> Conv2D 40 (act) -> SpatialDropout2D(0.25) -> Conv2D 24 (act) -> Conv2D 3.  Slots are
    padded to a multiple of 8 channels, so 40 and 24 fill theirs; widths (37, 21) leave pad
    channels, where sigmoid and softplus (act(0) != 0) are non-zero."""
    x = _input(cin)
    h = kl.Conv2D(widths[0], 1, activation=act)(x)
    h = kl.SpatialDropout2D(0.25)(h)
    h = kl.Conv2D(widths[1], 1, activation=act)(h)
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(h)), seed)


def act_layers(act, cin=88, seed=2):
    """Activation(act) layers that cannot fold into their producer: one whose producer (a linear
    Conv2D) has a second consumer, and one after an Add.  act = 'ReLU' uses the ReLU layer."""
    def A():
        return kl.ReLU() if act == 'ReLU' else kl.Activation(act)
    x = _input(cin)
    h0 = kl.Conv2D(40, 1)(x)
    a1 = A()(h0)
    h1 = kl.Conv2D(40, 1)(kl.SpatialDropout2D(0.25)(a1))
    a2 = A()(kl.Add()([h0, h1]))
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(a2)), seed)


def residual(cin=96, seed=3):
    """Two Add blocks (dropout inside each) and one Average; the projection p is consumed three
    times (block 1's conv, block 1's Add, the Average), so its gradient accumulates."""
    x = _input(cin)
    p = kl.Conv2D(32, 1, activation='softsign')(x)
    y = kl.Conv2D(32, 1, activation='tanh')(kl.Conv2D(32, 1, activation='tanh')(p))
    r1 = kl.Activation('relu')(kl.Add()([p, kl.SpatialDropout2D(0.2)(y)]))
    y = kl.SpatialDropout2D(0.1)(kl.Conv2D(32, 1, activation='elu')(r1))
    b2 = kl.Add()([r1, kl.Conv2D(32, 1, activation='softsign')(y)])
    av = kl.Average()([b2, p])
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(av)), seed)


def thin(cin=96, seed=4):
    """96 -> 32 -> 6 -> 16 -> 3: a layer with N <= 8 in the middle (thin forward, thin dIN and the
    per-thread dW accumulators)."""
    x = _input(cin)
    h = kl.Conv2D(32, 1, activation='tanh')(x)
    h = kl.Conv2D(6, 1, activation='softsign')(h)
    h = kl.Conv2D(16, 1, activation='tanh')(h)
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(h)), seed)


def layernorm(cin=96, seed=5):
    """Conv -> LayerNormalization (drawn gamma and beta) -> tanh -> Conv."""
    x = _input(cin)
    h = kl.LayerNormalization()(kl.Conv2D(40, 1)(x))
    h = kl.SpatialDropout2D(0.1)(kl.Activation('tanh')(h))
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(h)), seed)


def _flatten_hw(t):
    return t


def _reshape_back(ts):
    return ts[0]


def gated(cin=88, seed=6):
    """The SE gate and an MHA + LayerNorm block shaped like Model-88/attention_model.py's
    se_transformer_regr_head, at small widths.  Row-local on 1x1 maps only."""
    x = _input(cin)
    se = kl.GlobalAveragePooling2D()(x)
    se = kl.Dense(11, activation='relu')(se)
    se = kl.Dense(cin, activation='sigmoid')(se)
    g = kl.Multiply()([x, kl.Reshape((1, 1, cin))(se)])
    flat = kl.Lambda(_flatten_hw)(g)
    attn = kl.MultiHeadAttention(num_heads=2, key_dim=8)(flat, flat)
    h = kl.LayerNormalization()(kl.Add()([flat, attn]))
    ff = kl.Dense(cin)(kl.Dense(32, activation='relu')(h))
    h = kl.LayerNormalization()(kl.Add()([h, ff]))
    back = kl.Lambda(_reshape_back)([h, x])
    head = kl.Conv2D(24, 1, activation='relu')(back)
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(head)), seed)


def separable(cin=96, seed=7):
    """SeparableConv2D 1x1 (trained depthwise scale, pointwise GEMM) with an activation."""
    x = _input(cin)
    h = kl.SeparableConv2D(40, 1, activation='tanh')(x)
    h = kl.SeparableConv2D(24, 1, activation='softplus')(kl.SpatialDropout2D(0.25)(h))
    return _seeded(keras.Model(x, kl.Conv2D(3, 1)(h)), seed)


# the two large-program geometries, taken from the reference's checkpoints (tests/golden/models):
# 8equl7wt is 512-256-128-3 (208 dW blocks: two passes per step), 6togj6se an 11-layer residual
# tanh stack whose slot plan lives in device scratch
WIDE = {'npass': '8equl7wt', 'gslots': '6togj6se'}


def wide(which):
    return fixture(WIDE[which])


# name -> (builder, runs at P > 1)
GRAPHS = {}
for _a in ACTIVATIONS:
    GRAPHS['act_chain-' + _a] = (lambda a=_a: act_chain(a), True)
for _a in ('sigmoid', 'softplus', 'swish'):
    GRAPHS['act_chain_odd-' + _a] = (lambda a=_a: act_chain(a, widths=(37, 21)), True)
for _a in ACTIVATIONS + ('ReLU',):
    GRAPHS['act_layers-' + _a] = (lambda a=_a: act_layers(a), True)
GRAPHS.update({
    'residual': (residual, True),
    'thin': (thin, True),
    'layernorm': (layernorm, True),
    'gated': (gated, False),
    'separable': (separable, True),
    'wide-npass': (lambda: wide('npass'), False),    # ends in Flatten: rows only on 1x1 maps
    'wide-gslots': (lambda: wide('gslots'), True),
})


def build(name):
    return GRAPHS[name][0]()
