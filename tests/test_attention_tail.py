"""attn_tail_kernel of csrc/hpe_tail.hip (hpe_attn_tail / hpe_attn_tail_supported) on its own,
every instantiation tail_pick can return, against a plain reference.

The test packs its own parameter buffer from the layout documented at the top of hpe_tail.hip
(weight tiles in MFMA operand order, nine padded vectors, twenty descriptor words); a CPU test
holds that packer against hpe.spatial._mfma_order, so neither side is checked only against itself.

References, numpy, from the same fp32 inputs and parameters: a float64 evaluation of the chain as
the kernel's header comment writes it (LayerNorm over the first C features, biased variance, eps
inside the square root, activations through rowprog_emu._act), and an fp32 comparator of the same
formulas whose dot products and LayerNorm sums run strictly left to right, with a two-pass variance
and the activations evaluated on fp32 values.  Bound of every comparison, the rule of
tests/test_attention_kernels.py unchanged: with e32 = max |comparator - reference| over the case,

    |got - ref| <= max(4 e32, 4 * 2^-24 * max|ref|)   elementwise.

Every case has 304 rows (19 16-row blocks: three workgroups, the last one partly idle) unless its
point is the row count; those take their bound from the same data at 304 rows.  The CPU tests check
that the bound is never vacuous (<= 1e-3 max|ref| for every case), the hpe_attn_tail_supported table
and the host-side rejections; the GPU tests print err / max(e32, 2^-24 max|ref|) per case (<= 4
passes; the largest observed values are recorded in DESIGN.md, "Oracle and parity").
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import rowprog_emu as EMU
import util as U
from hpe import _lib
from hpe import spatial as SP
from test_attention_kernels import (DUMMY, ELU, F32, F64, HPE_EINVAL, HPE_OK, LEAKY_RELU, LINEAR, NULL, RELU, SELU,
                                    SENTINEL, SIGMOID, SOFTPLUS, SOFTSIGN, SWISH, TANH, _assert_close, _bound, _dev,
                                    _mha_case, _non_vacuous, _stream, _sum_l2r, _vp, needs_lib)

ACT_CODES = (LINEAR, TANH, RELU, SOFTSIGN, SIGMOID, ELU, SELU, SWISH, SOFTPLUS, LEAKY_RELU)
ACT_NAMES = ('linear', 'tanh', 'relu', 'softsign', 'sigmoid', 'elu', 'selu', 'swish', 'softplus', 'leaky_relu')

# descriptor words (the enum of csrc/hpe_tail.hip)
(TD_C, TD_HD, TD_FF, TD_HID, TD_ACT_FF, TD_ACT_HID, TD_ACT_OUT, TD_EPS1, TD_EPS2, TD_NW,
 TD_BO, TD_G1, TD_BE1, TD_BF1, TD_BF2, TD_G2, TD_BE2, TD_BC1, TD_BC2) = range(19)
TD_WORDS = 20
VEC_NAMES = ('bo', 'g1', 'be1', 'bf1', 'bf2', 'g2', 'be2', 'bc1', 'bc2')
ROWS = 304


def _blocks(n):
    return (n + 15) // 16


# ---------------------------------------------------------------------------------------------
# packer
# ---------------------------------------------------------------------------------------------
def _tile(w):
    """[K][N] -> [K/16][N/16][g][c][s] = W[16 bk + 4 g + s][16 bn + c], zero padded, one element
    index at a time."""
    K, N = w.shape
    kb, nb = _blocks(K), _blocks(N)
    out = np.zeros((kb, nb, 4, 16, 4), F32)
    for bk, bn, g, c, s in itertools.product(range(kb), range(nb), range(4), range(16), range(4)):
        k, n = 16 * bk + 4 * g + s, 16 * bn + c
        if k < K and n < N:
            out[bk, bn, g, c, s] = w[k, n]
    return out.ravel()


def _vec_lengths(C, FF, HID):
    """Padded length of the nine vectors, in buffer order."""
    return [16 * _blocks(n) for n in (C, C, C, FF, C, C, C, HID, 3)]


def _weight_floats(C, HD, FF, HID):
    cb, hb, fb, nhb = _blocks(C), _blocks(HD), _blocks(FF), _blocks(HID)
    return 256 * (hb * cb + cb * fb + fb * cb + cb * nhb + nhb)


def _f32_bits(x):
    return int(np.array([x], F32).view(np.int32)[0])


def _desc(C, HD, FF, HID, acts=(RELU, RELU, LINEAR), eps=(1e-3, 1e-3)):
    """The twenty descriptor words of a consistent buffer, as a list of ints."""
    d = [0] * TD_WORDS
    d[TD_C], d[TD_HD], d[TD_FF], d[TD_HID] = C, HD, FF, HID
    d[TD_ACT_FF], d[TD_ACT_HID], d[TD_ACT_OUT] = acts
    d[TD_EPS1], d[TD_EPS2] = _f32_bits(eps[0]), _f32_bits(eps[1])
    off = _weight_floats(C, HD, FF, HID)
    for i, n in enumerate(_vec_lengths(C, FF, HID)):
        d[TD_BO + i] = off
        off += n
    d[TD_NW] = off
    return d


def _cdesc(d):
    return (ctypes.c_int32 * TD_WORDS)(*d)


def _pack(p, acts, eps):
    """Parameters (dict of fp32 arrays) -> (descriptor words, parameter buffer)."""
    HD, C = p['wo'].shape
    FF, HID = p['wf1'].shape[1], p['wc1'].shape[1]
    d = _desc(C, HD, FF, HID, acts, eps)
    parts = [_tile(p[k]) for k in ('wo', 'wf1', 'wf2', 'wc1', 'wc2')]
    for name, n in zip(VEC_NAMES, _vec_lengths(C, FF, HID)):
        v = np.zeros(n, F32)
        v[:p[name].size] = p[name]
        parts.append(v)
    buf = np.concatenate(parts)
    assert buf.size == d[TD_NW] and buf.dtype == F32
    return d, buf


def test_packer_tiles_match_mfma_order():
    """CPU: the test's element-by-element tile packer and hpe.spatial._mfma_order agree bit for bit
    for K, N in {4, 16, 17, 88, 128}; the zero padding is really there and really zero."""
    rng = np.random.default_rng(7)
    for K in (4, 16, 17, 88, 128):
        for N in (4, 16, 17, 88, 128):
            w = (1.0 + rng.random((K, N))).astype(F32)   # no zero among the weights
            mine, theirs = _tile(w), SP._mfma_order(w, K, N)
            assert mine.shape == theirs.shape == (256 * _blocks(K) * _blocks(N),), (K, N)
            assert np.array_equal(mine.view(np.uint32), theirs.view(np.uint32)), (K, N)
            assert np.count_nonzero(theirs) == K * N, (K, N)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def _ref64(xg, o, p, acts, eps):
    """float64 evaluation of the chain in the header comment of csrc/hpe_tail.hip."""
    q = {k: v.astype(F64) for k, v in p.items()}

    def ln(x, g, b, e):
        mu = x.mean(axis=1, keepdims=True)
        var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
        return (x - mu) / np.sqrt(var + F64(F32(e))) * g + b
    t = xg.astype(F64) + o.astype(F64) @ q['wo'] + q['bo']
    u = ln(t, q['g1'], q['be1'], eps[0])
    v = EMU._act(acts[0], u @ q['wf1'] + q['bf1'])
    w = u + (v @ q['wf2'] + q['bf2'])
    z = ln(w, q['g2'], q['be2'], eps[1])
    h = EMU._act(acts[1], z @ q['wc1'] + q['bc1'])
    return np.asarray(EMU._act(acts[2], h @ q['wc2'] + q['bc2']), F64)


def _dot32(x, w):
    """fp32 x [R][K] . w [K][N], every dot product summed strictly left to right."""
    out = np.empty((x.shape[0], w.shape[1]), F32)
    for r0 in range(0, x.shape[0], 64):   # chunks of rows bound the (row, k, n) product array
        out[r0:r0 + 64] = _sum_l2r(x[r0:r0 + 64, :, None] * w[None], 1)
    return out


def _cmp32(xg, o, p, acts, eps):
    """fp32 comparator: the same formulas, sums left to right, two-pass variance."""
    C = xg.shape[1]

    def ln(x, g, b, e):
        mu = _sum_l2r(x, 1)[:, None] / F32(C)
        d = x - mu
        var = _sum_l2r(d * d, 1)[:, None] / F32(C)
        return d * (F32(1) / np.sqrt(var + F32(e))) * g + b

    def act(a, z):
        with np.errstate(over='ignore'):
            return np.asarray(EMU._act(a, z), F32)
    t = (_dot32(o, p['wo']) + p['bo']) + xg
    u = ln(t, p['g1'], p['be1'], eps[0])
    v = act(acts[0], _dot32(u, p['wf1']) + p['bf1'])
    w = u + (_dot32(v, p['wf2']) + p['bf2'])
    z = ln(w, p['g2'], p['be2'], eps[1])
    h = act(acts[1], _dot32(z, p['wc1']) + p['bc1'])
    y = act(acts[2], _dot32(h, p['wc2']) + p['bc2'])
    for a in (t, u, v, w, z, h, y):
        assert a.dtype == F32
    return y


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _params(C, HD, FF, HID, seed, affine=True, zero_bo=False):
    """Glorot-scaled kernels, biases of 0.1 N(0,1), gamma 1 + 0.1 N(0,1), beta 0.1 N(0,1)."""
    rng = np.random.default_rng([C, HD, FF, HID, seed])

    def kern(K, N):
        return (rng.standard_normal((K, N)) * np.sqrt(2.0 / (K + N))).astype(F32)

    def vec(n, mean=0.0):
        return (mean + 0.1 * rng.standard_normal(n)).astype(F32)
    p = {'wo': kern(HD, C), 'wf1': kern(C, FF), 'wf2': kern(FF, C), 'wc1': kern(C, HID), 'wc2': kern(HID, 3),
         'bo': vec(C), 'g1': vec(C, 1.0), 'be1': vec(C), 'bf1': vec(FF), 'bf2': vec(C), 'g2': vec(C, 1.0),
         'be2': vec(C), 'bc1': vec(HID), 'bc2': vec(3)}
    if not affine:   # scale=False / center=False LayerNorms: hpe/spatial.py packs ones and zeros
        p['g1'], p['g2'] = np.ones(C, F32), np.ones(C, F32)
        p['be1'], p['be2'] = np.zeros(C, F32), np.zeros(C, F32)
    if zero_bo:
        p['bo'] = np.zeros(C, F32)
    return p


REGIME_NAMES = ('moderate', 'offset', 'tiny', 'flat', 'noaffine')
FLAT_ROWS = slice(40, 104)   # four whole 16-row blocks and two partial ones


def _inputs(C, HD, regime, seed, rows=ROWS):
    """xg: post-ReLU-like features (tests/util.features); o: an attention output, 0.5 N(0,1)."""
    rng = np.random.default_rng([C, HD, seed, 11])
    xg = U.features(rows, C, seed=seed + 100 * C).reshape(rows, C)
    o = (0.5 * rng.standard_normal((rows, HD))).astype(F32)
    if regime == 'offset':      # mean far larger than the std
        xg = xg + F32(100.0)
    elif regime == 'tiny':
        xg, o = xg * F32(1e-3), o * F32(1e-3)
    elif regime == 'flat':      # rows whose pre-LayerNorm vector is constant (with bo = 0)
        n = FLAT_ROWS.stop - FLAT_ROWS.start
        xg[FLAT_ROWS] = rng.uniform(0.1, 1.0, (n, 1)).astype(F32)
        o[FLAT_ROWS] = 0.0
    return np.ascontiguousarray(xg, F32), np.ascontiguousarray(o, F32)


@functools.lru_cache(maxsize=None)
def _case(C, HD, FF, HID, acts=(RELU, RELU, LINEAR), eps=(1e-3, 1e-3), regime='moderate'):
    """One 304-row case: inputs, parameters, packed buffer, references.  Cached and never modified."""
    seed = 1 + REGIME_NAMES.index(regime)
    p = _params(C, HD, FF, HID, seed, affine=regime != 'noaffine', zero_bo=regime == 'flat')
    xg, o = _inputs(C, HD, regime, seed)
    d, buf = _pack(p, acts, eps)
    ref = _ref64(xg, o, p, acts, eps)
    cmp32 = _cmp32(xg, o, p, acts, eps)
    for a in (ref, cmp32):
        a.setflags(write=False)
    return {'C': C, 'HD': HD, 'FF': FF, 'HID': HID, 'xg': xg, 'o': o, 'p': p, 'acts': acts, 'eps': eps,
            'desc': d, 'w': buf, 'ref': ref, 'cmp': cmp32}


# every (HB, FB, NHB) tail_pick can return, at the lowest and the highest widths of its range
HD_LOW = {1: 4, 2: 20, 4: 52, 8: 116}
HD_HIGH = {1: 16, 2: 32, 4: 64, 8: 128}
FF_LOW, FF_HIGH = {2: 17, 4: 49}, {2: 32, 4: 64}
HID_LOW, HID_HIGH = {4: 49, 8: 113}, {4: 64, 8: 128}
FB_NHB = ((4, 8), (4, 4), (2, 8))
SWEEP = ([(84, HD_LOW[hb], FF_LOW[fb], HID_LOW[nhb]) for hb in (1, 2, 4, 8) for fb, nhb in FB_NHB]
         + [(96, HD_HIGH[hb], FF_HIGH[fb], HID_HIGH[nhb]) for hb in (1, 2, 4, 8) for fb, nhb in FB_NHB]
         + [(88, 52, 49, 113), (92, 20, 17, 113)])

REGIME_GEOM = (88, 64, 64, 64)
# (regime, eps1, eps2): zero-variance rows with eps 1e-3 only (at 1e-6 the fp32 comparator's own
# error makes the bound vacuous); the last two have eps1 != eps2
REGIMES = [(r, e, e) for r in ('moderate', 'offset', 'tiny', 'noaffine') for e in (1e-3, 1e-6)] + [
    ('flat', 1e-3, 1e-3), ('moderate', 1e-3, 1e-6), ('moderate', 1e-6, 1e-3)]

ACT_GEOM = (88, 16, 17, 113)   # FF and HID leave padded units: act(0) != 0 under sigmoid / softplus
BASE_ACTS = (RELU, RELU, LINEAR)
ACT_RUNS = [(pos, a) for pos in range(3) for a in ACT_CODES]

ROWS_GEOM = (92, 20, 49, 49)
ROW_COUNTS = (1, 15, 16, 17, 127, 128, 129)


def _acts_at(pos, a):
    acts = list(BASE_ACTS)
    acts[pos] = a
    return tuple(acts)


XG_GEOM = dict(C=88, n=8, P=35, H=4, D=16, FF=64, HID=64)   # 5 x 7 maps, 280 rows


@functools.lru_cache(maxsize=None)
def _pipeline_case():
    """hpe_mha_xg with C = 0 feeding the tail: references of the tail applied to the float64
    attention output (comparator: to the fp32 attention comparator's)."""
    g = XG_GEOM
    m = _mha_case('mfma', g['D'], g['P'], g['H'], 'moderate', n=g['n'])
    C, HD = g['C'], g['H'] * g['D']
    rows = g['n'] * g['P']
    p = _params(C, HD, g['FF'], g['HID'], 9)
    xg, _ = _inputs(C, HD, 'moderate', 9, rows=rows)
    d, buf = _pack(p, BASE_ACTS, (1e-3, 1e-3))
    ref = _ref64(xg, m['ref'], p, BASE_ACTS, (1e-3, 1e-3))
    cmp32 = _cmp32(xg, m['cmp'], p, BASE_ACTS, (1e-3, 1e-3))
    return {'C': C, 'HD': HD, 'xg': xg, 'qkv': m['qkv'], 'desc': d, 'w': buf, 'ref': ref, 'cmp': cmp32}


def _all_cases():
    out = [('sweep C=%d HD=%d FF=%d HID=%d' % g, _case(*g)) for g in SWEEP]
    out += [('regime %s eps %g/%g' % r, _case(*REGIME_GEOM, eps=r[1:], regime=r[0])) for r in REGIMES]
    out += [('act %s at %d' % (ACT_NAMES[a], pos), _case(*ACT_GEOM, acts=_acts_at(pos, a))) for pos, a in ACT_RUNS]
    out += [('rows', _case(*ROWS_GEOM)), ('strides C=84', _case(84, 52, 49, 113)), ('pipeline', _pipeline_case())]
    return out


def test_tail_references_are_not_vacuous():
    """CPU: for every GPU case (the row-count cases through the 304-row data they take their bound
    from) both references are finite and the bound is at most 1e-3 max|ref|; the cases have the
    structure they are meant to have."""
    bad = []
    for what, c in _all_cases():
        msg = _non_vacuous(c['ref'], c['cmp'])
        if msg:
            bad.append('%s: %s' % (what, msg))
    assert not bad, '\n'.join(bad)
    # all twelve instantiations, both C ends, and the two inner C
    inst = {(_blocks(g[1]), _blocks(g[2]), _blocks(g[3])) for g in SWEEP}
    assert inst == {(hb, fb, nhb) for hb in (1, 2, 4, 8) for fb, nhb in FB_NHB}
    for C in (84, 96):
        assert {(_blocks(g[1]), _blocks(g[2]), _blocks(g[3])) for g in SWEEP if g[0] == C} == inst
    assert {g[0] for g in SWEEP} == {84, 88, 92, 96}
    # flat rows: the pre-LayerNorm vector is constant, so the first LayerNorm returns beta exactly
    c = _case(*REGIME_GEOM, regime='flat')
    t = c['xg'].astype(F64) + c['o'].astype(F64) @ c['p']['wo'].astype(F64) + c['p']['bo']
    assert (t[FLAT_ROWS].std(axis=1) == 0).all() and (t.std(axis=1) > 0.1).sum() == ROWS - 64
    # offset: |mean| > 100 std in every row
    c = _case(*REGIME_GEOM, regime='offset')
    assert (np.abs(c['xg'].mean(axis=1)) > 100 * c['xg'].std(axis=1)).all()
    # the padded units of FF = 17 and HID = 113 are alive under sigmoid / softplus: act(0) >= 0.5
    assert ACT_GEOM[2] % 16 and ACT_GEOM[3] % 16
    for a in (SIGMOID, SOFTPLUS):
        assert float(EMU._act(a, np.float64(0))) >= 0.5
    # a LayerNorm whose variance also counts the padded features 84..87 (d = -mu there), the sum the
    # kernel's `< C` mask prevents, is far outside the bound
    c = _case(84, 52, 49, 113)
    t = c['xg'].astype(F64) + c['o'].astype(F64) @ c['p']['wo'].astype(F64) + c['p']['bo']
    mu, var = t.mean(axis=1), t.var(axis=1)
    rel = np.abs(np.sqrt((var + 1e-3) / (var + 4 * mu * mu / 84 + 1e-3)) - 1).max()
    assert rel > 1e-3 > 100 * _bound(c['ref'], c['cmp'])[0] / np.abs(c['ref']).max()


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _launch(xg, o, desc, w, n_rows, ld_xg=None, ld_o=None):
    """hpe_attn_tail on device tensors; y has 16 extra rows of SENTINEL that must stay untouched."""
    import torch
    lib = _lib.load()
    cd = _cdesc(desc)
    assert lib.hpe_attn_tail_supported(cd) == 1, desc
    y = torch.full((n_rows + 16, 3), SENTINEL, device='cuda')
    rc = lib.hpe_attn_tail(_vp(xg), xg.shape[1] if ld_xg is None else ld_xg, _vp(o),
                           o.shape[1] if ld_o is None else ld_o, n_rows, cd, _vp(w), _vp(y), _stream())
    assert rc == HPE_OK, 'rc %d: %s' % (rc, lib.hpe_last_error().decode(errors='replace'))
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert (got[n_rows:] == SENTINEL).all(), 'rows past n_rows written'
    return got[:n_rows]


def _run(c, what):
    got = _launch(_dev(c['xg']), _dev(c['o']), c['desc'], _dev(c['w']), c['xg'].shape[0])
    _assert_close(got, c['ref'], c['cmp'], 'hpe_attn_tail ' + what)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('C,HD,FF,HID', SWEEP)
def test_tail_every_instantiation(C, HD, FF, HID):
    _run(_case(C, HD, FF, HID), '<6,%d,%d,%d> C=%d HD=%d FF=%d HID=%d'
         % (_blocks(HD), _blocks(FF), _blocks(HID), C, HD, FF, HID))


@pytest.mark.gpu
@pytest.mark.parametrize('regime,eps1,eps2', REGIMES)
def test_tail_regimes(regime, eps1, eps2):
    _run(_case(*REGIME_GEOM, eps=(eps1, eps2), regime=regime), '%s eps %g/%g' % (regime, eps1, eps2))


@pytest.mark.gpu
@pytest.mark.parametrize('pos,act', ACT_RUNS, ids=['%s-%s' % (('ff', 'hid', 'out')[p], ACT_NAMES[a])
                                                   for p, a in ACT_RUNS])
def test_tail_activations(pos, act):
    _run(_case(*ACT_GEOM, acts=_acts_at(pos, act)), 'act %s at %s' % (ACT_NAMES[act], ('ff', 'hid', 'out')[pos]))


@pytest.mark.gpu
@pytest.mark.parametrize('n_rows', ROW_COUNTS)
def test_tail_row_counts(n_rows):
    """xg and o are allocated at exactly n_rows (the kernel clamps row loads to the last row); the
    bound is the one of the same data at 304 rows."""
    c = _case(*ROWS_GEOM)
    got = _launch(_dev(c['xg'][:n_rows]), _dev(c['o'][:n_rows]), c['desc'], _dev(c['w']), n_rows)
    bound, e32, floor = _bound(c['ref'], c['cmp'])
    err = float(np.abs(got.astype(F64) - c['ref'][:n_rows]).max())
    print('hpe_attn_tail n_rows=%d: err %.3g, e32 %.3g, floor %.3g, err / max(e32, floor) = %.3f'
          % (n_rows, err, e32, floor, err / max(e32, floor)))
    assert np.isfinite(got).all()
    assert err <= bound, 'n_rows=%d: max err %.3g > bound %.3g' % (n_rows, err, bound)


@pytest.mark.gpu
def test_tail_grid_wrap():
    """More 16-row blocks than 8 waves x one workgroup per CU: the block loop takes a second trip.
    The rows are the 304-row case tiled, so row i must equal row i mod 304 of the small run bit for
    bit (304 is a multiple of 16: a row keeps its lane)."""
    import torch
    c = _case(*REGIME_GEOM)
    small = _run(c, 'grid wrap, 304 rows')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 128 * cus + 133
    reps = -(-n // ROWS)
    xg, o = _dev(c['xg']).repeat(reps, 1)[:n].contiguous(), _dev(c['o']).repeat(reps, 1)[:n].contiguous()
    got = _launch(xg, o, c['desc'], _dev(c['w']), n)
    want = np.tile(small, (reps, 1))[:n]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        'rows differ: first at %d' % int(np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize('C,HD,FF,HID,pad_xg,pad_o', [(88, 64, 64, 64, 8, 4), (84, 52, 49, 113, 4, 4)])
def test_tail_strides(C, HD, FF, HID, pad_xg, pad_o):
    """Row strides above the widths, the padding columns NaN: bit-identical to the dense call."""
    c = _case(C, HD, FF, HID)
    dense = _run(c, 'dense C=%d' % C)
    xg = np.concatenate([c['xg'], np.full((ROWS, pad_xg), np.nan, F32)], axis=1)
    o = np.concatenate([c['o'], np.full((ROWS, pad_o), np.nan, F32)], axis=1)
    got = _launch(_dev(xg), _dev(o), c['desc'], _dev(c['w']), ROWS, ld_xg=C + pad_xg, ld_o=HD + pad_o)
    assert np.array_equal(got.view(np.uint32), dense.view(np.uint32))


@pytest.mark.gpu
def test_tail_after_mha_xg_null_xg():
    """The pipeline's call: o from hpe_mha_xg with C = 0 and a null xg on 5 x 7 maps, then the tail."""
    import torch
    lib = _lib.load()
    g, c = XG_GEOM, _pipeline_case()
    rows = g['n'] * g['P']
    qkv = _dev(c['qkv'])
    o = torch.full((rows, c['HD']), SENTINEL, device='cuda')
    rc = lib.hpe_mha_xg(_vp(qkv), qkv.shape[1], NULL, 0, _vp(o), c['HD'], g['n'], g['P'], g['H'], g['D'], _stream())
    assert rc == HPE_OK, lib.hpe_last_error()
    got = _launch(_dev(c['xg']), o, c['desc'], _dev(c['w']), rows)
    _assert_close(got, c['ref'], c['cmp'], 'hpe_mha_xg (C = 0) -> hpe_attn_tail')


# ---------------------------------------------------------------------------------------------
# host side (no GPU: pointers are DUMMY and n_rows = 0, so nothing is ever launched on them)
# ---------------------------------------------------------------------------------------------
GRID_C = (4, 16, 64, 80, 84, 85, 86, 88, 90, 92, 96, 100, 112, 128)
GRID_HD = (4, 8, 12, 16, 18, 20, 32, 34, 36, 48, 52, 64, 68, 80, 96, 112, 116, 128, 132, 144, 160)
GRID_F = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 96, 97, 112, 113, 128, 129, 144)


def _documented(C, HD, FF, HID):
    return (C in (84, 88, 92, 96) and HD % 4 == 0 and _blocks(HD) in (1, 2, 4, 8)
            and (_blocks(FF), _blocks(HID)) in FB_NHB)


@needs_lib
def test_tail_supported_table():
    """hpe_attn_tail_supported is 1 exactly on the documented set; all twelve instantiations are in
    it (every one launches on an MI355X: test_tail_every_instantiation)."""
    lib = _lib.load()
    wrong, ones = [], set()
    for C, HD, FF, HID in itertools.product(GRID_C, GRID_HD, GRID_F, GRID_F):
        got = lib.hpe_attn_tail_supported(_cdesc(_desc(C, HD, FF, HID)))
        if got != int(_documented(C, HD, FF, HID)):
            wrong.append((C, HD, FF, HID, got))
        if got:
            ones.add((_blocks(C), _blocks(HD), _blocks(FF), _blocks(HID)))
    assert not wrong, wrong[:20]
    assert ones == {(6, hb, fb, nhb) for hb in (1, 2, 4, 8) for fb, nhb in FB_NHB}
    for g in SWEEP + [REGIME_GEOM, ACT_GEOM, ROWS_GEOM]:
        assert lib.hpe_attn_tail_supported(_cdesc(_desc(*g))) == 1, g


def _tail(lib, d, ld_xg=None, ld_o=None, n_rows=0, xg=DUMMY, o=DUMMY, w=DUMMY, y=DUMMY):
    ld_xg = d[TD_C] if ld_xg is None else ld_xg
    ld_o = d[TD_HD] if ld_o is None else ld_o
    return lib.hpe_attn_tail(xg, ld_xg, o, ld_o, n_rows, _cdesc(d) if d is not None else NULL, w, y, NULL)


@needs_lib
def test_tail_rejections():
    lib = _lib.load()
    d = _desc(88, 64, 64, 64)
    assert _tail(lib, d) == HPE_OK                    # n_rows = 0
    assert _tail(lib, d, ld_xg=96, ld_o=68) == HPE_OK
    assert lib.hpe_attn_tail_supported(NULL) == 0
    assert lib.hpe_attn_tail(DUMMY, 88, DUMMY, 64, 0, NULL, DUMMY, DUMMY, NULL) == HPE_EINVAL
    for k in ('xg', 'o', 'w', 'y'):
        assert _tail(lib, d, **{k: NULL}) == HPE_EINVAL, k
        assert b'hpe_attn_tail' in lib.hpe_last_error()
    for kw in (dict(ld_xg=87), dict(ld_xg=84), dict(ld_o=63), dict(ld_o=60), dict(ld_xg=90), dict(ld_o=66)):
        assert _tail(lib, d, **kw) == HPE_EINVAL, kw
        msg = lib.hpe_last_error()
        assert b'strides' in msg and b'%d' % kw.get('ld_xg', 88) in msg and b'%d' % kw.get('ld_o', 64) in msg, msg
    bad = list(d)
    bad[TD_FF] = 16
    assert _tail(lib, bad) == HPE_EINVAL


def _with(d, word, value):
    d = list(d)
    d[word] = value
    return d


@needs_lib
@pytest.mark.parametrize('geom', [(88, 64, 64, 64), (84, 4, 17, 113), (96, 128, 64, 128)])
def test_tail_descriptor_validation(geom):
    """Words the kernel would trust: activation codes, the nine vector offsets, TD_NW and the eps
    words.  Each bad value is refused by hpe_attn_tail_supported and is HPE_EINVAL from
    hpe_attn_tail; the values next to them are accepted."""
    lib = _lib.load()
    C, HD, FF, HID = geom
    good = _desc(*geom)
    wend, lens = _weight_floats(*geom), _vec_lengths(C, FF, HID)
    assert good[TD_NW] == wend + sum(lens)

    def ok(d):
        r = lib.hpe_attn_tail_supported(_cdesc(d))
        assert _tail(lib, d) == (HPE_OK if r else HPE_EINVAL)
        if not r:
            assert b'hpe_attn_tail' in lib.hpe_last_error()
        return r
    assert ok(good) == 1
    for word in (TD_ACT_FF, TD_ACT_HID, TD_ACT_OUT):
        for a in ACT_CODES:
            assert ok(_with(good, word, a)) == 1, (word, a)
        for a in (-1, LEAKY_RELU + 1, 255, -2 ** 31, 2 ** 31 - 1):
            assert ok(_with(good, word, a)) == 0, (word, a)
    for i, n in enumerate(lens):
        word = TD_BO + i
        assert ok(_with(good, word, wend)) == 1, i                   # lowest legal offset
        assert ok(_with(good, word, good[TD_NW] - n)) == 1, i        # highest legal offset
        for off in (-4, -1, 0, wend - 4, good[word] + 1, good[word] + 2, good[TD_NW] - n + 4, good[TD_NW],
                    2 ** 31 - 4, -2 ** 31):
            assert ok(_with(good, word, off)) == 0, (i, off)
    # a larger buffer is fine (hpe_attn_tail stages TD_NW floats), up to the LDS; a smaller one is not
    assert ok(_with(good, TD_NW, good[TD_NW] + 4)) == 1
    for nw in (good[TD_NW] - 4, good[TD_NW] + 2, wend, 0, -4, 160 * 256 + 4, 2 ** 31 - 4):
        assert ok(_with(good, TD_NW, nw)) == 0, nw
    for word in (TD_EPS1, TD_EPS2):
        for e in (1e-3, 1e-6, 1e-12, 1.0, 1e-40):
            assert ok(_with(good, word, _f32_bits(e))) == 1, e
        for e in (0.0, -0.0, -1e-3, np.inf, -np.inf, np.nan):
            assert ok(_with(good, word, _f32_bits(e))) == 0, e
        assert ok(_with(good, word, 0x7FC00001)) == 0    # a NaN with payload
        assert ok(_with(good, word, -1)) == 0            # 0xFFFFFFFF, a negative NaN


def test_tail_plan_descriptors_pass_validation():
    """The test's descriptor layout is the one hpe/spatial.py:_attn_tail writes: same offsets,
    TD_NW and eps bits for a graph's geometry (so the plan's descriptors pass the same checks)."""
    mc, w = U.fixture('12uei1sn')
    plan = SP.SpatialPlan(mc, w)
    d = [int(v) for v in plan.tail['desc']]
    mine = _desc(d[TD_C], d[TD_HD], d[TD_FF], d[TD_HID], acts=tuple(d[TD_ACT_FF:TD_ACT_OUT + 1]),
                 eps=(np.array([d[TD_EPS1]], np.int32).view(F32)[0], np.array([d[TD_EPS2]], np.int32).view(F32)[0]))
    assert mine == d
    assert plan.tail['w'].size == d[TD_NW]
