"""The image-level attention-stage kernels of csrc/hpe_spatial.hip, each against a plain reference.

hpe_mha / hpe_mha_xg (softmax(q k^T) v per image and head, MFMA core for key_dim <= 32 and VALU
core above it or under HPE_MHA_VALU), hpe_se_gate (mean -> dense -> act -> dense -> act ->
multiply) and hpe_seg_mean (per-image row mean), called through ctypes on torch device tensors.

References, numpy, from the same fp32 inputs: a float64 evaluation, and an fp32 comparator of the
same formula whose sums run left to right (np.cumsum(..., dtype=float32)[-1]), so its summation
order is no better than a kernel's.  Bound of every comparison (assert_fp32_parity's rule of
tests/test_spatial.py, without the LayerNorm floor): with e32 = max |comparator - reference|,

    |got - ref| <= max(4 e32, 4 * 2^-24 * max|ref|)   elementwise;

the second term is the floor where the comparator happens to be exact (P = 1: the output is v).
The CPU tests check that this bound is never vacuous (<= 1e-3 max|ref| for every case) and the
host-side argument validation; the GPU tests print err / max(e32, 2^-24 max|ref|) per case (<= 4
passes; the largest observed values are recorded in DESIGN.md, "Oracle and parity").
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import rowprog_emu as EMU
from hpe import _lib

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
HPE_OK, HPE_EINVAL = 0, 1
SENTINEL = -12345.0
DUMMY = ctypes.c_void_p(4096)   # non-null, never dereferenced: every call that takes it is rejected
NULL = ctypes.c_void_p(0)       # on the host or has n_images = 0

# activation codes of csrc/hpe_prog.h (rowprog_emu._act takes the same numbers)
LINEAR, TANH, RELU, SOFTSIGN, SIGMOID, ELU, SELU, SWISH, SOFTPLUS, LEAKY_RELU = range(10)


def _sum_l2r(a, axis):
    """fp32 sum along `axis`, strictly left to right."""
    return np.take(np.cumsum(a, axis=axis, dtype=F32), -1, axis=axis)


def _bound(ref, cmp32):
    """(bound, e32, floor) of one case."""
    e32 = float(np.abs(cmp32.astype(F64) - ref).max())
    floor = EPS * float(np.abs(ref).max())
    return max(4.0 * e32, 4.0 * floor), e32, floor


def _non_vacuous(ref, cmp32):
    bound, e32, _ = _bound(ref, cmp32)
    top = float(np.abs(ref).max())
    if not (np.isfinite(ref).all() and np.isfinite(cmp32).all()):
        return 'reference not finite'
    if not bound <= 1e-3 * top:
        return 'bound %.3g > 1e-3 * max|ref| = %.3g (e32 %.3g)' % (bound, 1e-3 * top, e32)
    return None


def _assert_close(got, ref, cmp32, what):
    bound, e32, floor = _bound(ref, cmp32)
    err = float(np.abs(got.astype(F64) - ref).max())
    ratio = err / max(e32, floor)
    print('%s: err %.3g, e32 %.3g, floor %.3g, err / max(e32, floor) = %.3f' % (what, err, e32, floor, ratio))
    assert np.isfinite(got).all(), what
    assert err <= bound, ('%s: max err %.3g > bound %.3g (e32 %.3g, max|ref| %.3g): err / e32 = %.2f, needs '
                          'factor %.2f' % (what, err, bound, e32, np.abs(ref).max(), err / e32 if e32 else np.inf,
                                           ratio))


# ---------------------------------------------------------------------------------------------
# hpe_mha / hpe_mha_xg
# ---------------------------------------------------------------------------------------------
MFMA_KB, VALU_KB = 128, 256   # keys per LDS block of the two cores (MHAM_KB, MHA_KB)
REGIMES = ('moderate', 'peaked', 'wide')

# (core, HPE_MHA_VALU forced, D, P, H)
MHA_CASES = (
    [('mfma', False, D, P, 3) for D, P in [(1, 1), (1, 33), (2, 128), (7, 129), (16, 160), (31, 255), (32, 257),
                                           (5, 300)]]
    + [('valu', True, D, P, 3) for D, P in [(1, 35), (3, 256), (20, 257), (28, 64), (32, 300)]]
    + [('valu', False, D, P, 3) for D, P in [(33, 64), (40, 257), (48, 300), (57, 33), (64, 256), (64, 513)]]
    + [('mfma', False, 7, 129, 1), ('mfma', False, 16, 160, 5), ('valu', False, 40, 257, 1),
       ('valu', True, 28, 64, 5)])
# hpe_mha_xg: (core, forced, D, P, H, C); C = 0 goes with a null xg (the attention-tail call)
XG_CASES = [('mfma', False, 7, 129, 3, 8), ('mfma', False, 16, 160, 3, 0),
            ('valu', False, 40, 257, 3, 8), ('valu', True, 20, 257, 3, 0)]


def _mha_refs(q, k, v):
    """q, k, v (n, H, P, D) fp32 -> float64 reference and fp32 comparator, (n * P, H * D) rows."""
    n, H, P, D = q.shape
    s = q.astype(F64) @ k.astype(F64).transpose(0, 1, 3, 2)
    a = np.exp(s - s.max(-1, keepdims=True))
    a /= a.sum(-1, keepdims=True)
    ref = a @ v.astype(F64)
    s32 = np.matmul(q, k.transpose(0, 1, 3, 2))
    p32 = np.exp(s32 - s32.max(-1, keepdims=True))
    assert s32.dtype == F32 and p32.dtype == F32
    l32 = _sum_l2r(p32, -1)
    o32 = np.empty((n, H, P, D), F32)
    for b in range(n):
        for h in range(H):
            for q0 in range(0, P, 64):   # chunks of queries bound the (query, key, d) product array
                o32[b, h, q0:q0 + 64] = _sum_l2r(p32[b, h, q0:q0 + 64, :, None] * v[b, h][None], 1)
    cmp32 = o32 / l32[..., None]
    assert cmp32.dtype == F32
    rows = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(n * P, H * D)  # noqa: E731
    return rows(ref), rows(cmp32), s


def _planted_positions(P):
    pos = []
    for p in (0, 31, 32, 127, 128, P - 1):
        if p < P and p not in pos:
            pos.append(p)
    return pos


@functools.lru_cache(maxsize=None)
def _mha_case(core, D, P, H, regime, n=2, C=8):
    """One case: fp32 inputs (different data per image and head), references, regime statistics."""
    rng = np.random.default_rng([D, P, H, REGIMES.index(regime), n])
    q = rng.standard_normal((n, H, P, D)) * D ** -0.25
    k = rng.standard_normal((n, H, P, D)) * D ** -0.25
    v = rng.standard_normal((n, H, P, D))
    stats = {}
    if regime == 'peaked':
        # planted keys of norm 4 on a circle (D = 1: +4 / -4), every other key of norm ~0.5; query i
        # points at planted key (i + image * H + head) mod m with gain 6: its score is 24, the
        # next planted key's 24 cos(2 pi / m) <= 12, any other key's ~3
        pos = _planted_positions(P)
        m = len(pos)
        ndir = min(m, 2) if D == 1 else m   # one dimension holds two directions: rotate the pair
        k = rng.standard_normal((n, H, P, D)) * 0.5 / np.sqrt(D)
        q = rng.standard_normal((n, H, P, D)) * 0.1 / np.sqrt(D)
        want = np.zeros((n, H, P), np.int64)
        for b in range(n):
            for h in range(H):
                for j in range(ndir):
                    u = np.zeros(D)
                    if D == 1:
                        u[0] = 1.0 if j == 0 else -1.0
                    else:
                        u[0], u[1] = np.cos(2 * np.pi * j / ndir), np.sin(2 * np.pi * j / ndir)
                    at = pos[(j + b * H + h) % m]
                    k[b, h, at] = 4.0 * u
                    q[b, h, j::ndir] += 6.0 * u
                    want[b, h, j::ndir] = at
        stats['want'] = want
    elif regime == 'wide':
        # keys of the first 32-key sub-block damped to a quarter and of the rest of the first LDS
        # block to a half, so a query's largest score mostly comes later and the running-max
        # rescaling (corr) does real work; q scaled so the scores span +-90 (exp(90) overflows fp32)
        kb = MFMA_KB if core == 'mfma' else VALU_KB
        w = np.where(np.arange(P) < 32, 0.25, np.where(np.arange(P) < kb, 0.5, 1.0))
        k = k * w[None, None, :, None]
        s0 = q @ k.transpose(0, 1, 3, 2)
        q = q * (90.0 / np.abs(s0).max(axis=(2, 3), keepdims=True))
    q, k, v = (np.ascontiguousarray(t, dtype=F32) for t in (q, k, v))
    ref, cmp32, s = _mha_refs(q, k, v)
    arg = s.argmax(-1)
    stats['argmax'] = arg
    stats['span'] = float(np.abs(s).max())
    top2 = np.sort(s, axis=-1)[..., -2:]
    stats['gap'] = float((top2[..., 1] - top2[..., 0]).min()) if P > 1 else np.inf
    rows = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(n * P, H * D)  # noqa: E731
    qkv = np.concatenate([rows(q), rows(k), rows(v)], axis=1)
    x = rng.standard_normal((n * P, C)).astype(F32)
    return {'n': n, 'P': P, 'H': H, 'D': D, 'C': C, 'x': x, 'qkv': qkv, 'ref': ref, 'cmp': cmp32,
            'stats': stats, 'core': core}


def _sweep_case(D, core):
    return _mha_case(core, D, 3, 1, 'moderate', n=1)


def test_mha_references_are_not_vacuous():
    """CPU: for every hpe_mha / hpe_mha_xg case the references are finite and the bound is at most
    1e-3 max|ref|; the peaked and wide-range inputs have the structure they are meant to have."""
    bad = []
    cases = [(c, D, P, H, r, 2) for c, _, D, P, H in MHA_CASES for r in REGIMES]
    cases += [(c, D, P, H, r, 2) for c, _, D, P, H, _ in XG_CASES for r in REGIMES]
    cases += [('mfma', D, 3, 1, 'moderate', 1) for D in range(1, 33)]
    cases += [('valu', D, 3, 1, 'moderate', 1) for D in range(1, 65)]
    for core, D, P, H, regime, n in dict.fromkeys(cases):
        c = _mha_case(core, D, P, H, regime, n=n)
        what = '%s D=%d P=%d H=%d %s' % (core, D, P, H, regime)
        msg = _non_vacuous(c['ref'], c['cmp'])
        if msg:
            bad.append('%s: %s' % (what, msg))
        st = c['stats']
        if regime == 'peaked':
            # the planted key wins every query by a margin of >= 8 in the score (weight ratio e^-8)
            if not (np.array_equal(st['argmax'], st['want']) and st['gap'] >= 8.0):
                bad.append('%s: planted keys do not dominate (gap %.2f)' % (what, st['gap']))
            if P > 1 and len(np.unique(st['want'])) < min(len(_planted_positions(P)), 2 if D == 1 else 6):
                bad.append('%s: planted positions not all used' % what)
        if regime == 'wide':
            if not 89.0 <= st['span'] <= 91.0:
                bad.append('%s: scores span %.1f' % (what, st['span']))
            kb = MFMA_KB if core == 'mfma' else VALU_KB
            if P >= 64 and (st['argmax'] >= 32).mean() < 0.75:
                bad.append('%s: largest score after the first sub-block for only %.2f of the queries'
                           % (what, (st['argmax'] >= 32).mean()))
            if P >= kb + 32 and (st['argmax'] >= kb).mean() < 0.25:
                bad.append('%s: largest score after the first block for only %.2f of the queries'
                           % (what, (st['argmax'] >= kb).mean()))
    assert not bad, '\n'.join(bad)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else NULL


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run_mha(case, what, entry='hpe_mha', C=None):
    """Launch one case and check: return code, value bound, pass-through columns bit for bit,
    sentinel in the slack columns of every output row."""
    import torch
    lib = _lib.load()
    n, P, H, D = case['n'], case['P'], case['H'], case['D']
    C = case['C'] if C is None else C
    HD = H * D
    x = case['x'][:, :C]
    slack = np.full((n * P, 5), np.nan, F32)   # never read: a NaN would poison the output
    out = torch.full((n * P, C + HD + 3), SENTINEL, device='cuda')
    if entry == 'hpe_mha':
        inp = _dev(np.concatenate([x, case['qkv'], slack], axis=1))
        assert inp.shape[1] == C + 3 * HD + 5
        rc = lib.hpe_mha(_vp(inp), inp.shape[1], C, _vp(out), out.shape[1], n, P, H, D, _stream())
    else:
        inp = _dev(np.concatenate([case['qkv'], slack], axis=1))
        xg = _dev(x) if C > 0 else None
        rc = lib.hpe_mha_xg(_vp(inp), inp.shape[1], _vp(xg), C, _vp(out), out.shape[1], n, P, H, D, _stream())
    assert rc == HPE_OK, '%s: rc %d: %s' % (what, rc, lib.hpe_last_error().decode(errors='replace'))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :C].view(np.uint32), x.view(np.uint32)), what + ': pass-through columns'
    assert (got[:, C + HD:] == SENTINEL).all(), what + ': slack columns written'
    _assert_close(got[:, C:C + HD], case['ref'], case['cmp'], what)


def _set_core(monkeypatch, forced):
    if forced:
        monkeypatch.setenv('HPE_MHA_VALU', '1')
    else:
        monkeypatch.delenv('HPE_MHA_VALU', raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('core,forced,D,P,H', MHA_CASES)
def test_mha_matches_reference(core, forced, D, P, H, regime, monkeypatch):
    _set_core(monkeypatch, forced)
    _run_mha(_mha_case(core, D, P, H, regime), 'hpe_mha %s D=%d P=%d H=%d %s' % (core, D, P, H, regime))


@pytest.mark.gpu
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('core,forced,D,P,H,C', XG_CASES)
def test_mha_xg_matches_reference(core, forced, D, P, H, C, regime, monkeypatch):
    _set_core(monkeypatch, forced)
    _run_mha(_mha_case(core, D, P, H, regime), 'hpe_mha_xg %s D=%d P=%d C=%d %s' % (core, D, P, C, regime),
             entry='hpe_mha_xg', C=C)


@pytest.mark.gpu
@pytest.mark.parametrize('D', range(1, 65))
def test_mha_every_key_dim_launches(D, monkeypatch):
    """Every 1 <= key_dim <= 64 runs on the default path (MFMA core to 32, VALU core above)."""
    _set_core(monkeypatch, False)
    core = 'mfma' if D <= 32 else 'valu'
    _run_mha(_sweep_case(D, core), 'hpe_mha sweep %s D=%d' % (core, D))


@pytest.mark.gpu
@pytest.mark.parametrize('D', range(1, 33))
def test_mha_every_key_dim_launches_valu(D, monkeypatch):
    """... and every key_dim <= 32 on the VALU core under HPE_MHA_VALU."""
    _set_core(monkeypatch, True)
    _run_mha(_sweep_case(D, 'valu'), 'hpe_mha sweep valu (forced) D=%d' % D)


def _mha(lib, D=4, P=4, H=3, C=8, ld_in=None, ld_out=None, inp=DUMMY, n=0):
    ld_in = C + 3 * H * D if ld_in is None else ld_in
    ld_out = C + H * D if ld_out is None else ld_out
    return lib.hpe_mha(inp, ld_in, C, DUMMY, ld_out, n, P, H, D, NULL)


@needs_lib
def test_mha_rejections():
    """Host-side validation, no device needed: each bad argument is HPE_EINVAL (also for an empty
    batch, so nothing is ever launched on the dummy pointers); every 1 <= D <= 64 is accepted."""
    lib = _lib.load()
    assert _mha(lib) == HPE_OK
    assert _mha(lib, D=0) == HPE_EINVAL
    assert _mha(lib, D=65) == HPE_EINVAL
    assert _mha(lib, ld_in=8 + 3 * 3 * 4 - 1) == HPE_EINVAL
    assert _mha(lib, ld_out=8 + 3 * 4 - 1) == HPE_EINVAL
    assert _mha(lib, P=0) == HPE_EINVAL
    assert _mha(lib, H=0) == HPE_EINVAL
    assert _mha(lib, inp=NULL) == HPE_EINVAL
    assert b'hpe_mha' in lib.hpe_last_error()
    for D in range(1, 65):
        assert _mha(lib, D=D) == HPE_OK, D
        assert lib.hpe_mha_xg(DUMMY, 3 * 3 * D, DUMMY, 8, DUMMY, 8 + 3 * D, 0, 4, 3, D, NULL) == HPE_OK, D
    assert lib.hpe_mha_xg(DUMMY, 3 * 3 * 65, DUMMY, 8, DUMMY, 8 + 3 * 65, 0, 4, 3, 65, NULL) == HPE_EINVAL


# ---------------------------------------------------------------------------------------------
# hpe_se_gate
# ---------------------------------------------------------------------------------------------
SE_N = 3
SE_SHAPES = [(4, 1, 1), (88, 11, 35), (96, 12, 256), (64, 7, 300), (512, 512, 5), (256, 3, 2304)]
# (C, U, P, act1, act2, b1 null, b2 null): relu / sigmoid (the reference's pair) on every shape,
# then every other accepted code once as act1 and once as act2, one null b1, one null b2
SE_RUNS = [s + (RELU, SIGMOID, False, False) for s in SE_SHAPES] + [
    (4, 1, 1, LINEAR, TANH, False, False),
    (88, 11, 35, TANH, SOFTSIGN, True, False),
    (96, 12, 256, SOFTSIGN, ELU, False, True),
    (64, 7, 300, ELU, SELU, False, False),
    (512, 512, 5, SELU, SOFTPLUS, False, False),
    (512, 512, 5, SOFTPLUS, LEAKY_RELU, False, False),
    (256, 3, 2304, LEAKY_RELU, LINEAR, False, False),
]


@functools.lru_cache(maxsize=None)
def _rows_data(n, P, C, seed):
    """(n, P, C) fp32 rows whose per-image, per-channel means differ by O(0.1)."""
    rng = np.random.default_rng([n, P, C, seed])
    return (0.5 * rng.standard_normal((n, P, C)) + 0.3 * rng.standard_normal((n, 1, C))).astype(F32)


@functools.lru_cache(maxsize=None)
def _se_case(C, U, P, act1, act2, no_b1, no_b2):
    x = _rows_data(SE_N, P, C, 1)
    rng = np.random.default_rng([C, U, P, 2])
    w1 = (rng.standard_normal((C, U)) * 2.0 / np.sqrt(C)).astype(F32)
    w2 = (rng.standard_normal((U, C)) * 2.0 / np.sqrt(U)).astype(F32)
    b1 = None if no_b1 else (0.5 + 0.3 * rng.standard_normal(U)).astype(F32)   # relu units mostly alive
    b2 = None if no_b2 else (0.3 * rng.standard_normal(C)).astype(F32)

    def gate(mean, dt):
        z1 = mean @ w1.astype(dt) + (0 if b1 is None else b1.astype(dt))
        hid = np.asarray(EMU._act(act1, z1), dtype=dt)
        z2 = hid @ w2.astype(dt) + (0 if b2 is None else b2.astype(dt))
        return np.asarray(EMU._act(act2, z2), dtype=dt)

    ref = x.astype(F64) * gate(x.astype(F64).mean(axis=1), F64)[:, None, :]
    g32 = gate(_sum_l2r(x, 1) / F32(P), F32)
    cmp32 = x * g32[:, None, :]
    assert g32.dtype == F32 and cmp32.dtype == F32
    return {'x': x, 'w1': w1, 'b1': b1, 'w2': w2, 'b2': b2, 'ref': ref.reshape(SE_N * P, C),
            'cmp': cmp32.reshape(SE_N * P, C)}


def test_se_gate_and_seg_mean_references_are_not_vacuous():
    bad = []
    for run in SE_RUNS:
        c = _se_case(*run)
        msg = _non_vacuous(c['ref'], c['cmp'])
        if msg:
            bad.append('se_gate %r: %s' % (run, msg))
        # the gates of two images differ by far more than the bound: a gate from the wrong image shows
        g = c['ref'].reshape(SE_N, -1, run[0])[:, 0, :] / c['x'][:, 0, :].astype(F64)
        if min(np.abs(g[i] - g[j]).max() for i, j in ((0, 1), (0, 2), (1, 2))) < 1e-2:
            bad.append('se_gate %r: images have the same gate' % (run,))
    for C, P in SEG_CASES:
        ref, cmp32 = _seg_refs(C, P)
        msg = _non_vacuous(ref, cmp32)
        if msg:
            bad.append('seg_mean C=%d P=%d: %s' % (C, P, msg))
    assert not bad, '\n'.join(bad)
    used1 = {r[3] for r in SE_RUNS}
    used2 = {r[4] for r in SE_RUNS}
    every = set(range(10)) - {SWISH}
    assert every - {SIGMOID} <= used1 and every - {RELU} <= used2
    assert any(r[5] for r in SE_RUNS) and any(r[6] for r in SE_RUNS)


@pytest.mark.gpu
@pytest.mark.parametrize('C,U,P,act1,act2,no_b1,no_b2', SE_RUNS)
def test_se_gate_matches_reference(C, U, P, act1, act2, no_b1, no_b2):
    import torch
    lib = _lib.load()
    c = _se_case(C, U, P, act1, act2, no_b1, no_b2)
    x = _dev(c['x'].reshape(SE_N * P, C))
    xg = torch.full_like(x, SENTINEL)
    w1, w2 = _dev(c['w1']), _dev(c['w2'])
    b1 = None if no_b1 else _dev(c['b1'])
    b2 = None if no_b2 else _dev(c['b2'])
    rc = lib.hpe_se_gate(_vp(x), _vp(xg), SE_N, P, C, _vp(w1), _vp(b1), U, act1, _vp(w2), _vp(b2), act2, _stream())
    assert rc == HPE_OK, lib.hpe_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), c['x'].reshape(SE_N * P, C))
    _assert_close(xg.cpu().numpy(), c['ref'], c['cmp'],
                  'hpe_se_gate C=%d U=%d P=%d act %d/%d b1 %s b2 %s' % (C, U, P, act1, act2, not no_b1, not no_b2))


def _se(lib, P=4, C=8, U=2, act1=RELU, act2=SIGMOID, w1=DUMMY):
    return lib.hpe_se_gate(DUMMY, DUMMY, 0, P, C, w1, NULL, U, act1, DUMMY, NULL, act2, NULL)


@needs_lib
def test_se_gate_rejections():
    lib = _lib.load()
    assert _se(lib) == HPE_OK
    assert _se(lib, C=512, U=512) == HPE_OK
    assert _se(lib, C=6) == HPE_EINVAL
    assert _se(lib, C=516) == HPE_EINVAL
    assert _se(lib, U=513) == HPE_EINVAL
    assert _se(lib, P=0) == HPE_EINVAL
    for bad in (-1, LEAKY_RELU + 1, SWISH):   # the entry point rejects swish today: pinned
        assert _se(lib, act1=bad) == HPE_EINVAL, bad
        assert _se(lib, act2=bad) == HPE_EINVAL, bad
    assert _se(lib, w1=NULL) == HPE_EINVAL
    assert b'hpe_se_gate' in lib.hpe_last_error()


# ---------------------------------------------------------------------------------------------
# hpe_seg_mean
# ---------------------------------------------------------------------------------------------
SEG_CASES = [(1, 1), (3, 2304), (96, 64), (255, 7), (256, 300)]


def _seg_refs(C, P):
    x = _rows_data(SE_N, P, C, 3)
    return x.astype(F64).mean(axis=1), _sum_l2r(x, 1) / F32(P)


@pytest.mark.gpu
@pytest.mark.parametrize('C,P', SEG_CASES)
def test_seg_mean_matches_reference(C, P):
    import torch
    lib = _lib.load()
    ref, cmp32 = _seg_refs(C, P)
    x = _dev(_rows_data(SE_N, P, C, 3).reshape(SE_N * P, C))
    y = torch.full((SE_N + 1, C), SENTINEL, device='cuda')
    rc = lib.hpe_seg_mean(_vp(x), _vp(y), SE_N, P, C, _stream())
    assert rc == HPE_OK, lib.hpe_last_error()
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert (got[SE_N] == SENTINEL).all()
    _assert_close(got[:SE_N], ref, cmp32, 'hpe_seg_mean C=%d P=%d' % (C, P))


@needs_lib
def test_seg_mean_rejections():
    lib = _lib.load()
    assert lib.hpe_seg_mean(DUMMY, DUMMY, 0, 4, 256, NULL) == HPE_OK
    assert lib.hpe_seg_mean(DUMMY, DUMMY, 0, 4, 257, NULL) == HPE_EINVAL
    assert lib.hpe_seg_mean(DUMMY, DUMMY, 0, 4, 0, NULL) == HPE_EINVAL
    assert lib.hpe_seg_mean(DUMMY, DUMMY, 0, 0, 4, NULL) == HPE_EINVAL
    assert b'hpe_seg_mean' in lib.hpe_last_error()
