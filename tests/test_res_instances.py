"""CPU: the case matrix of tests/res_stacks.py covers the residual-stack dispatch (csrc/hpe_res.hip
res_pick).  BASE must reach every compiled kernel instance, so that tests/test_gpu_res_instances.py,
which holds each case to the float64 oracle, holds every instance: a new instance fails this test
until the matrix reaches it.  Instance ids are taken from the program words with
hpe_res_fit_multi_instance_words (host arithmetic, no device call)."""
import ctypes

import numpy as np
import pytest

import res_stacks as RS
from hpe import _lib, compiler

N_INSTANCES = 32     # 2 input widths x (fast | runtime) x 4 block counts x (bottleneck | none)


def _compile(mc, w, P=1):
    return compiler.compile_graph(mc, w, mode='train', P=P)


def _instance(prog):
    w = np.ascontiguousarray(prog.words, np.int32)
    return _lib.load().hpe_res_fit_multi_instance_words(w.ctypes.data_as(ctypes.c_void_p), w.size)


@pytest.fixture(scope='module')
def programs():
    return {name: _compile(*RS.build(name)) for name in RS.CASES}


def test_base_cases_cover_every_instance(programs):
    ids = {}
    for name in RS.BASE:
        kw = RS.CASES[name]
        prog = programs[name]
        assert prog.kind == 'res', name
        inst = _instance(prog)
        fast = kw['act'] == 'softsign'
        assert inst == RS.instance_id(kw['cin'], fast, kw['blocks'], kw['bottleneck']), name
        ids[name] = inst
    assert set(ids.values()) == set(range(N_INSTANCES)), ids
    assert len(ids) == N_INSTANCES


def test_edge_cases_run_the_runtime_instances(programs):
    for name in RS.EDGE:
        kw = RS.CASES[name]
        prog = programs[name]
        assert prog.kind == 'res', name
        inst = _instance(prog)
        assert 0 <= inst < N_INSTANCES, name
        assert (inst >> 3) & 1 == 0, (name, inst)          # the `fast` bit
        assert inst == RS.instance_id(kw['cin'], False, kw['blocks'], kw['bottleneck']), name


def test_info_reports_the_geometry(programs):
    for name, kw in RS.CASES.items():
        info = programs[name].info
        assert info['blocks'] == kw['blocks'], name
        assert info['bottleneck'] == kw['bottleneck'], name
        assert info['layers'] == 2 * kw['blocks'] + 2 + (1 if kw['bottleneck'] else 0), name


@pytest.mark.parametrize('P', [9, 25])
def test_every_case_is_a_res_program_on_maps(P):
    for name in RS.CASES:
        assert _compile(*RS.build(name), P=P).kind == 'res', name


def test_stacks_outside_the_family_fall_back_to_the_generic_program():
    # swish's derivative needs the pre-activation (compiler.NEEDS_Z), which the kernel does not keep
    for kw in (dict(act='swish', post='relu'), dict(act='tanh', post='swish')):
        prog = _compile(*RS.stack(cin=88, blocks=2, bottleneck=8, dr=0.1, **kw))
        assert prog.kind == 'generic', kw
        assert _instance(prog) == -1
    # an input width no kernel is compiled for
    prog = _compile(*RS.stack(cin=92, blocks=2, bottleneck=8, act='softsign', post='relu', dr=0.1))
    assert prog.kind == 'generic'
    assert _instance(prog) == -1


def test_drawn_weights_and_no_bias():
    mc, w = RS.build('edge-softplus-nobias')
    assert w and not any(k.endswith('/bias') for k in w)
    mc, w = RS.build('88-softsign-nb3-bot8')
    first = next(v for k, v in w.items() if v.ndim == 4 and v.shape[2] == 88)
    assert 0.9 < first.std() < 1.1
    assert any(k.endswith('/bias') and np.abs(v).max() > 0.1 for k, v in w.items())
    drops = [l for l in mc['config']['layers'] if l['class_name'] == 'SpatialDropout2D']
    assert len(drops) == 1 + 2 * 3 + 1
    assert not [l for l in RS.build('edge-leaky-bot13')[0]['config']['layers']
                if l['class_name'] == 'SpatialDropout2D']
