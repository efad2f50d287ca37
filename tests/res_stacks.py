"""Narrow residual stacks for the fused residual-stack kernel tests — TEST INFRASTRUCTURE, not a test.

stack() builds, over hpe.keras, the family csrc/hpe_res.hip trains (hpe/compiler.py _try_res):

    x (cin) -> Conv2D 16 (act) + drop -> blocks x [Conv2D 16 (act) + drop -> Conv2D 16 (act) + drop ->
    Add(block input) -> Activation(post)] -> [Conv2D bottleneck (act) + drop] -> Conv2D 3 (out_act) [+ drop]

and returns (model_config, weights) with drawn weights, by the rule of synth_graphs._seeded: a
first-layer kernel of unit variance, later kernels of std 2 / sqrt(fan_in), biases N(0, 0.3), so the
pre-activations have both signs and reach the saturating parts of the activations (Glorot weights
and zero biases leave every layer in its linear region).

BASE is one stack per compiled kernel instance (res_pick: input width, block count, bottleneck,
compile-time "fast" against runtime activations); EDGE holds runtime-instance stacks that each reach
a layer option BASE does not.  tests/test_res_instances.py asserts that BASE covers the dispatch.
"""
from hpe import keras
from synth_graphs import _seeded

kl = keras.layers


def stack(cin, blocks, bottleneck, act, post, out_act=None, dr=0.1, out_dr=0.0, bias=True, reg=0.0, seed=1):
    """(model_config, weights).  dr = 0 emits no dropout layers; reg: l2 on every kernel."""
    keras.backend.clear_session()
    l2 = keras.regularizers.l2(reg) if reg else None

    def conv(units, a, x, rate):
        y = kl.Conv2D(filters=units, kernel_size=1, padding='same', activation=a, use_bias=bias,
                      kernel_regularizer=l2)(x)
        return kl.SpatialDropout2D(rate)(y) if rate else y

    inp = keras.Input(shape=(None, None, cin))
    x = conv(16, act, inp, dr)
    for _ in range(blocks):
        y = conv(16, act, conv(16, act, x, dr), dr)
        x = kl.Activation(post)(kl.Add()([x, y]))
    if bottleneck:
        x = conv(bottleneck, act, x, dr)
    return _seeded(keras.Model(inp, conv(3, out_act, x, out_dr)), seed)


def instance_id(cin, fast, blocks, bottleneck):
    """csrc/hpe_res.hip res_pick's instance id."""
    return (((1 if cin == 96 else 0) * 2 + (1 if fast else 0)) * 4 + (blocks - 1)) * 2 + (1 if bottleneck else 0)


# name -> stack() arguments
BASE = {}
for _cin in (88, 96):
    for _act in ('softsign', 'tanh'):         # softsign / relu / bottleneck 0 | 8: the fast instances
        for _nb in (1, 2, 3, 4):
            for _bot in (0, 8):
                BASE['%d-%s-nb%d-bot%d' % (_cin, _act, _nb, _bot)] = dict(
                    cin=_cin, blocks=_nb, bottleneck=_bot, act=_act, post='relu', dr=0.1)

EDGE = {
    # pad lanes of a narrow bottleneck under act(0) != 0, a linear post-add, a non-linear dropped-out output
    'edge-sigmoid-bot5': dict(cin=88, blocks=2, bottleneck=5, act='sigmoid', post='linear', out_act='tanh',
                              dr=0.1, out_dr=0.2),
    # a full-width bottleneck and a post-add activation that is not piecewise linear
    'edge-elu-bot16': dict(cin=96, blocks=1, bottleneck=16, act='elu', post='sigmoid', dr=0.3),
    # a one-unit bottleneck and no bias anywhere
    'edge-softplus-nobias': dict(cin=88, blocks=3, bottleneck=1, act='softplus', post='tanh', dr=0.1, bias=False),
    # no dropout words at all, at the deepest stack
    'edge-leaky-bot13': dict(cin=96, blocks=4, bottleneck=13, act='leaky_relu', post='selu', dr=0.0),
    # the smallest instance, relu kinks everywhere
    'edge-relu-min': dict(cin=88, blocks=1, bottleneck=0, act='relu', post='relu', dr=0.2),
}

CASES = dict(BASE)
CASES.update(EDGE)
assert len(BASE) == 32 and len(CASES) == 37


def build(name, **over):
    """(model_config, weights) of a named case; each case draws its weights from its own seed."""
    kw = dict(CASES[name], seed=100 + list(CASES).index(name))
    kw.update(over)
    return stack(**kw)
