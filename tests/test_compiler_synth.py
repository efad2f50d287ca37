"""CPU: the compiler's 'train' lowering of the synthetic graphs of tests/synth_graphs.py, executed
by the numpy emulator of the kernel semantics (tests/rowprog_emu.py), against the oracle's autodiff
at test_compiler.py's bars.  P = 1 and P = 9 (3x3 maps: SpatialDropout masks shared by the 9 rows of
an image, labels broadcast over positions), n = 7 images, so 63 rows at P = 9: ragged against every
tile height.  A wrong gradient on the GPU (test_gpu_rowprog_grad.py) with this test passing is a
wrong kernel, not a wrong lowering."""
import numpy as np
import pytest

import hpe.compiler as C
import rowprog_emu as EMU
import synth_graphs as SG
from oracle import keras_ref as K
from util import features, input_channels, labels

N_IMG = 7
CASES = [(name, P) for name, (_, spatial) in SG.GRAPHS.items() for P in ((1, 9) if spatial else (1,))]


def _flat(prog, w):
    p = np.zeros(prog.n_params)
    for k, (o, shp) in prog.param_index.items():
        p[o:o + int(np.prod(shp))] = w[k].ravel()
    p[prog.n_train:] = prog.consts
    return p


@pytest.mark.parametrize('name,P', CASES)
def test_emulated_train_program_matches_oracle(name, P):
    mc, w = SG.build(name)
    c = input_channels(mc)
    assert c in (88, 96)
    side = int(round(P ** 0.5))
    x = features(N_IMG, c, seed=len(name), h=side, w=side)
    y = labels(N_IMG, seed=P)
    pt = C.compile_graph(mc, w, 'train', P=P, fused=False)
    assert pt.kind == 'generic' and pt.C_out == 3
    assert (N_IMG * P) % pt.T != 0
    r = EMU.run(pt, _flat(pt, w), x.reshape(N_IMG * P, c), P=P, y_img=y.astype(np.float64),
                inv_count=1.0 / (N_IMG * P * 3), seed=77)
    g = K.Graph(mc, w)
    grads, _, _ = K.gradients(g, x, y, drop_seed=77)
    assert set(grads) == set(pt.param_index)
    for k, (o, shp) in pt.param_index.items():
        ref_g = grads[k].numpy().ravel() - 2 * g.l2[k] * g.params[k].numpy().ravel()
        got = r['grad'][o:o + int(np.prod(shp))]
        np.testing.assert_allclose(got, ref_g, rtol=1e-6, atol=1e-9 + 1e-6 * np.abs(ref_g).max(), err_msg=k)
    p = g.forward(x, training=True, drop_seed=77).detach().numpy().reshape(N_IMG, P, 3)
    e = p - y.reshape(N_IMG, 1, 3).astype(np.float64)
    np.testing.assert_allclose(r['sse'], (e * e).sum(), rtol=1e-9)
    np.testing.assert_allclose(r['sae'], np.abs(e).sum(), rtol=1e-9)


def test_emulated_image_offset():
    """The dropout masks follow the launch's image offset (a data-parallel rank's share of a
    batch): the emulated program at img_off = 1000 against the oracle at image_offset = 1000."""
    mc, w = SG.build('act_chain-tanh')
    x = features(N_IMG, 96, seed=1, h=3, w=3)
    y = labels(N_IMG, seed=2)
    pt = C.compile_graph(mc, w, 'train', P=9, fused=False)
    r = EMU.run(pt, _flat(pt, w), x.reshape(N_IMG * 9, 96), P=9, y_img=y.astype(np.float64),
                inv_count=1.0 / (N_IMG * 27), seed=5, img_off=1000)
    from util import oracle_step
    g64, sse, sae = oracle_step(mc, w, x, y, pt, 5, image_offset=1000)
    np.testing.assert_allclose(r['grad'], g64, rtol=1e-6, atol=1e-9 + 1e-6 * np.abs(g64).max())
    g0 = oracle_step(mc, w, x, y, pt, 5)[0]
    assert np.abs(g0 - g64).max() > 1e-3 * np.abs(g64).max()    # the offset does change the masks
    np.testing.assert_allclose([r['sse'], r['sae']], [sse, sae], rtol=1e-9)


def test_synthetic_graphs_reach_what_they_are_for():
    """The program features each builder exists for are in its compiled program (so a compiler
    change that stops emitting them shows here, not as silently lost coverage)."""
    def prog(name, P=1):
        return C.compile_graph(*SG.build(name), 'train', P=P, fused=False)

    def ops(p):
        w = p.words.astype(np.int64)
        oo = int(w[C.H_OPS_OFF])
        return [w[oo + C.O_WORDS * i: oo + C.O_WORDS * (i + 1)] for i in range(int(w[C.H_NOPS]))]

    def slots(p):
        w = p.words.astype(np.int64)
        so = int(w[C.H_SLOTS_OFF])
        return [w[so + 4 * i: so + 4 * i + 4] for i in range(int(w[C.H_NSLOTS]))]

    types = lambda p: {int(o[C.O_TYPE]) for o in ops(p)}
    # pad channels: slots of 40 / 24 channels have none, those of 37 / 21 do
    assert all(int(s[1]) == int(s[2]) for s in slots(prog('act_chain-sigmoid')) if int(s[1]) in (40, 24))
    assert any(int(s[1]) == 37 and int(s[2]) == 40 for s in slots(prog('act_chain_odd-sigmoid')))
    assert any(int(s[1]) == 21 and int(s[2]) == 24 for s in slots(prog('act_chain_odd-sigmoid')))
    # swish keeps its pre-activation, in the fused epilogue and as a stand-alone layer
    for name in ('act_chain-swish', 'act_chain_odd-swish', 'act_layers-swish'):
        assert any(int(o[C.O_EZ]) >= 0 for o in ops(prog(name))), name
    for name in ('act_chain-tanh', 'act_layers-tanh'):
        assert all(int(o[C.O_EZ]) < 0 for o in ops(prog(name))), name
    # stand-alone Activation layers: forward as OP_EW with an activation; their backward rides on
    # the dIN that produces the gradient (DST_EPIGRAD).  The stand-alone OP_EPIGRAD appears where a
    # gradient is complete only after an accumulation: in the residual graph
    for name in ('act_layers-ReLU', 'act_layers-sigmoid'):
        o_ = ops(prog(name))
        assert sum(int(o[C.O_TYPE]) == C.OP_EW and int(o[C.O_EACT]) > 0 for o in o_) == 2, name
        assert any(int(o[C.O_TYPE]) in (C.OP_DIN, C.OP_TDIN) and int(o[C.O_MODE]) == C.DST_EPIGRAD for o in o_)
    p = prog('residual')
    assert C.OP_EPIGRAD in types(p)
    assert any(int(o[C.O_TYPE]) == C.OP_DIN and int(o[C.O_MODE]) == C.DST_ACCUM for o in ops(p)) or \
        any(int(o[C.O_TYPE]) == C.OP_EWB and int(o[C.O_MODE]) != 0 for o in ops(p))
    p = prog('thin')
    assert {C.OP_TDENSE, C.OP_TDIN} <= types(p)
    assert any(int(o[C.O_TYPE]) == C.OP_TACC and int(o[C.O_AUX3]) == C.TACC_GEMM for o in ops(p))
    for P in (1, 9):
        p = prog('layernorm', P)
        assert {C.OP_LN, C.OP_LNB} <= types(p)
        assert any(int(o[C.O_TYPE]) == C.OP_TACC and int(o[C.O_AUX3]) == C.TACC_DIAG for o in ops(p))
    p = prog('gated')
    assert any(int(o[C.O_TYPE]) == C.OP_EW and int(o[C.O_FLAGS]) & C.EW_MUL for o in ops(p))
    assert {C.OP_LN, C.OP_LNB} <= types(p)
    p = prog('separable')
    assert any(int(o[C.O_TYPE]) == C.OP_EW and int(o[C.O_FLAGS]) & C.EW_AFFINE for o in ops(p))
    assert int(prog('wide-npass').words[C.H_NPASS]) > 1
    assert int(prog('wide-gslots').words[C.H_GSLOTS]) == 1


@pytest.mark.parametrize('name', [n for n, (_, spatial) in SG.GRAPHS.items() if not spatial])
def test_graphs_refused_on_maps(name):
    """Pinned refusals: the SE gate / single-token MHA and a Flatten head are row-local on 1x1
    maps only, so these graphs have no P = 9 case."""
    mc, w = SG.build(name)
    with pytest.raises(ValueError, match=r'row-local only on 1x1 feature maps \(P == 1\)'):
        C.compile_graph(mc, w, 'train', P=9, fused=False)
