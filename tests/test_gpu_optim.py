"""GPU: the three kernels every per-step training path ends in (csrc/hpe_rowprog.hip reduce_kernel,
optim_kernel, reduce_optim_kernel), called directly through the C ABI on device tensors.  No model
is involved; hpe_reduce takes its slab geometry from a program handle (a small act_chain engine).

hpe_reduce is held bit for bit to a numpy float32 restatement of the documented summation order,
and to the float64 sum within grid * 2^-24 * sum |ws_i|.  hpe_optim_step is held to a float64
restatement of oracle/keras_ref.py LegacyOptimizer on the same float32 inputs (hyper-parameters
included: the kernel receives them as floats).  Its margin is measured, not chosen: the same
formulas in numpy float32 against float64, worst element per optimizer, in units of
2^-24 * (|w| + |step|) for w and 2^-24 * |value| for m and v; the kernel gets 4 x that (summation /
contraction order differs), with a floor of 1 unit.  Measured on the inputs below (worst over the
four sizes and four iterations), numpy float32 restatement:
    SGD     w 2.16
    Adam    w 3.97   m 3.88   v 6.71
    Adamax  w 4.19   m 3.83   v 1.95
(The gradient, the moments and the weight of one element share a sign, as they do up to noise on
a descent path, so that no element's g = graw * gscale + 2 l2 w or m + (g - m)(1 - b1) cancels
and the units stay meaningful; the weights themselves are of both signs.)"""
import ctypes

import numpy as np
import pytest
import torch

import hpe.compiler as C
import synth_graphs as SG
from hpe import _lib
from hpe._lib import ptr
from hpe.engine import Engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRIDS = (1, 3, 4, 5, 13, 16, 17, 33)
SGD, ADAM, ADAMAX = 0, 1, 2
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope='module')
def prog():
    mc, w = SG.build('act_chain-tanh')
    eng = Engine(mc, w, fused=False)
    c = eng.program('train', 1)
    assert c.prog.kind == 'generic'
    return eng, c


def _rows(c, grid):
    rows = grid * c.prog.T - 5
    assert _lib.load().hpe_launch_grid(c.h, rows) == grid
    return rows


def _mixed(rng, shape):
    """Mixed sign, magnitudes log-uniform over 1e-6 .. 1e3."""
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-6, 3, size=shape)).astype(np.float32)


def _reduce_ref(ws):
    """The documented order in float32: wave w sums slabs w, w+4, ... into four strided
    accumulators (a 16-slab unrolled loop, then a tail into the first), (s0+s1)+(s2+s3) per wave,
    (p0+p1)+(p2+p3) over the waves."""
    grid, n = ws.shape
    part = []
    for w in range(4):
        s = [np.zeros(n, np.float32) for _ in range(4)]
        g = w
        while g + 12 < grid:
            for j in range(4):
                s[j] = s[j] + ws[g + 4 * j]
            g += 16
        while g < grid:
            s[0] = s[0] + ws[g]
            g += 4
        part.append((s[0] + s[1]) + (s[2] + s[3]))
    return (part[0] + part[1]) + (part[2] + part[3])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('grid', GRIDS)
def test_reduce_order_bound_and_guard(prog, grid):
    eng, c = prog
    lib = _lib.load()
    n = eng.n_train + 4
    slab = int(c.prog.words[C.H_SLAB])
    assert slab >= n
    rows = _rows(c, grid)
    assert lib.hpe_workspace_size(c.h, rows) == grid * slab * 4
    ws = _mixed(np.random.default_rng(grid), (grid, slab))
    wsd = torch.from_numpy(ws).cuda()
    guard = 64
    grad = torch.full((n + guard,), -7.25, dtype=torch.float32, device='cuda')
    _lib.check(lib.hpe_reduce(c.h, rows, ptr(wsd), ptr(grad), _lib.stream()), 'hpe_reduce')
    got = grad.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(_reduce_ref(ws[:, :n])))
    s64 = ws[:, :n].astype(np.float64).sum(0)
    bound = grid * U * np.abs(ws[:, :n].astype(np.float64)).sum(0)
    assert (np.abs(got[:n] - s64) <= bound).all()
    assert np.all(got[n:] == -7.25)                       # words past n_train + 4 are not written

    # the fused reduce + optimizer launch: the same gradient bit for bit, the loss sums in regp,
    # and the weights of hpe_optim_step applied to hpe_reduce's gradient
    nt = eng.n_train
    rng = np.random.default_rng(100 + grid)
    st = {k: torch.from_numpy(v).cuda() for k, v in _optim_inputs(rng, nt).items()}
    hp = (2.8e-4, 0.9, 0.999, 1e-7, 3, 0.5)
    ogrid = lib.hpe_optim_grid(nt)
    a = {k: v.clone() for k, v in st.items()}
    grad2 = torch.full((n + guard,), -7.25, dtype=torch.float32, device='cuda')
    regp2 = torch.zeros(2 + ogrid, dtype=torch.float32, device='cuda')
    _lib.check(lib.hpe_reduce_optim_step(c.h, rows, ptr(wsd), ptr(grad2), ADAM, *hp, ptr(a['w']), ptr(a['wt']),
                                         ptr(a['m']), ptr(a['v']), ptr(a['l2']), ptr(a['tpos']), nt, ptr(regp2),
                                         _lib.stream()), 'hpe_reduce_optim_step')
    got2 = grad2.cpu().numpy()
    assert np.array_equal(_bits(got2), _bits(got))
    r2 = regp2.cpu().numpy()
    assert np.array_equal(_bits(r2[:2]), _bits(got[nt:nt + 2]))
    b = {k: v.clone() for k, v in st.items()}
    regp = torch.zeros(2 + ogrid, dtype=torch.float32, device='cuda')
    _lib.check(lib.hpe_optim_step(ADAM, *hp, ptr(b['w']), ptr(b['wt']), ptr(b['m']), ptr(b['v']), ptr(grad),
                                  ptr(b['l2']), ptr(b['tpos']), nt, ptr(regp), _lib.stream()), 'hpe_optim_step')
    for k in ('w', 'wt', 'm', 'v'):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(_bits(regp.cpu().numpy()), _bits(r2))


def _optim_inputs(rng, n):
    """w of both signs; m of w's sign; v >= 0; l2 per element with zeros among it; tpos a
    permutation with about a quarter of its entries at -1; wt sentinel words."""
    w = (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-3, 1, size=n)).astype(np.float32)
    m = (np.sign(w) * 10.0 ** rng.uniform(-4, 1, size=n)).astype(np.float32)
    v = (10.0 ** rng.uniform(-6, 2, size=n)).astype(np.float32)
    l2 = np.where(rng.random(n) < 0.4, 0.0, 10.0 ** rng.uniform(-6, -1, size=n)).astype(np.float32)
    tpos = rng.permutation(n).astype(np.int32)
    tpos[rng.random(n) < 0.25] = -1
    wt = np.full(n, 123.5, np.float32)
    return {'w': w, 'm': m, 'v': v, 'l2': l2, 'tpos': tpos, 'wt': wt}


def _grad_input(rng, w):
    """Gradient words (+ 4 trailing loss words) of w's sign, magnitudes over 1e-5 .. 1e2, with one
    block of exact zeros (there m and v are zeroed too)."""
    n = w.size
    g = (np.sign(w) * 10.0 ** rng.uniform(-5, 2, size=n)).astype(np.float32)
    z0, z1 = n // 3, min(n, n // 3 + 40)
    g[z0:z1] = 0.0
    return np.concatenate([g, np.asarray([5.0, 3.0, 0.0, 0.0], np.float32)]), (z0, z1)


def _step(kind, dt, w, m, v, graw, l2, lr, b1, b2, eps, it, gscale):
    """oracle/keras_ref.py LegacyOptimizer.apply on g = graw * gscale + 2 l2 w, in dtype dt.  The
    hyper-parameters are the floats the kernel receives; the bias correction is formed in double
    and rounded to dt, as the host does.  Returns (w, m, v, step)."""
    f = lambda a: np.asarray(a, dtype=dt)
    lr64, b164, b264 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    w, m, v, graw, l2 = f(w), f(m), f(v), f(graw), f(l2)
    lr_, b1_, b2_, eps_, gs_ = (dt(np.float32(q)) for q in (lr, b1, b2, eps, gscale))
    one, two = dt(1), dt(2)
    g = graw * gs_ + two * l2 * w
    if kind == SGD:
        step = lr_ * g
        return w - step, m, v, step
    m = m + (g - m) * (one - b1_)
    if kind == ADAM:
        v = v + (g * g - v) * (one - b2_)
        alpha = dt(lr64 * np.sqrt(1.0 - b264 ** it) / (1.0 - b164 ** it))
        step = (m * alpha) / (np.sqrt(v) + eps_)
    else:
        v = np.maximum(b2_ * v, np.abs(g))
        alpha = dt(lr64 / (1.0 - b164 ** it))
        step = alpha * (m / (v + eps_))
    return w - step, m, v, step


def _units(got, ref, scale):
    d = np.abs(np.asarray(got, np.float64) - ref)
    ok = scale > 0
    assert np.all(d[~ok] == 0)
    return float((d[ok] / (U * scale[ok])).max()) if ok.any() else 0.0


HYPER = {SGD: (0.05, 0.9, 0.999, 1e-7), ADAM: (2.8e-4, 0.9, 0.999, 1e-7), ADAMAX: (1e-3, 0.9, 0.999, 1e-7)}
NAMES = {SGD: 'sgd', ADAM: 'adam', ADAMAX: 'adamax'}


@pytest.mark.parametrize('n', [1, 255, 257, 300_001])
@pytest.mark.parametrize('kind', [SGD, ADAM, ADAMAX])
def test_optim_step_vs_float64_restatement(kind, n):
    """n = 300,001 is past 1024 x 256, so the grid-stride loop runs; iterations 1 .. 10^7 take the
    bias correction from its largest value to 1."""
    lib = _lib.load()
    lr, b1, b2, eps = HYPER[kind]
    gscale = 0.37
    ogrid = lib.hpe_optim_grid(n)
    assert (ogrid == 1024) == (n > 1024 * 256)
    for it in (1, 2, 1000, 10_000_000):
        rng = np.random.default_rng(1000 * kind + it % 997 + n)
        inp = _optim_inputs(rng, n)
        gbuf, (z0, z1) = _grad_input(rng, inp['w'])
        inp['m'][z0:z1] = 0.0
        inp['v'][z0:z1] = 0.0
        d = {k: torch.from_numpy(a.copy()).cuda() for k, a in inp.items()}
        gd = torch.from_numpy(gbuf).cuda()
        regp = torch.full((2 + ogrid + 8,), -7.25, dtype=torch.float32, device='cuda')
        null_mv = kind == SGD
        _lib.check(lib.hpe_optim_step(kind, lr, b1, b2, eps, it, gscale, ptr(d['w']), ptr(d['wt']),
                                      NULL if null_mv else ptr(d['m']), NULL if null_mv else ptr(d['v']),
                                      ptr(gd), ptr(d['l2']), ptr(d['tpos']), n, ptr(regp), _lib.stream()),
                   'hpe_optim_step')
        got = {k: t.cpu().numpy() for k, t in d.items()}
        args = (inp['w'], inp['m'], inp['v'], gbuf[:n], inp['l2'], lr, b1, b2, eps, it, gscale)
        w64, m64, v64, s64 = _step(kind, np.float64, *args)
        w32, m32, v32, _ = _step(kind, np.float32, *args)
        sw = np.abs(w64) + np.abs(s64)
        rows = [('w', got['w'], w32, w64, sw)]
        if kind != SGD:
            rows += [('m', got['m'], m32, m64, np.abs(m64)), ('v', got['v'], v32, v64, np.abs(v64))]
        for nm, g_, r32, r64, sc in rows:
            floor = _units(r32, r64, sc)
            err = _units(g_, r64, sc)
            print('%s n=%d iter=%d %s: kernel %.2f units, numpy float32 restatement %.2f units'
                  % (NAMES[kind], n, it, nm, err, floor))
            assert err <= max(1.0, 4.0 * floor), (nm, err, floor)
        if kind == SGD:     # m and v were null: nothing of theirs to compare; the inputs are untouched
            assert np.array_equal(got['m'], inp['m']) and np.array_equal(got['v'], inp['v'])
        # the zero block: no gradient and no history; without L2 the weight does not move
        zb = slice(z0, z1)
        still = inp['l2'][zb] == 0
        assert np.array_equal(got['w'][zb][still], inp['w'][zb][still])
        assert np.isfinite(got['w']).all() and np.isfinite(got['m']).all() and np.isfinite(got['v']).all()
        # the mirror: entries with tpos >= 0 hold the new weight, every other word is untouched
        has = inp['tpos'] >= 0
        assert np.array_equal(_bits(got['wt'][inp['tpos'][has]]), _bits(got['w'][has]))
        rest = np.ones(n, bool)
        rest[inp['tpos'][has]] = False
        assert np.all(got['wt'][rest] == 123.5)
        assert np.array_equal(got['l2'], inp['l2']) and np.array_equal(got['tpos'], inp['tpos'])
        # regp: the loss sums, then one L2 partial per block; words past them untouched
        r = regp.cpu().numpy()
        assert r[0] == 5.0 and r[1] == 3.0
        reg64 = float((inp['l2'].astype(np.float64) * inp['w'].astype(np.float64) ** 2).sum())
        np.testing.assert_allclose(r[2:2 + ogrid].astype(np.float64).sum(), reg64, rtol=1e-6)
        assert np.all(r[2 + ogrid:] == -7.25)


def test_optim_refusals(prog):
    """Pinned refusals of the two entry points (HPE_EINVAL -> ValueError), none of which launches."""
    eng, c = prog
    lib = _lib.load()
    n = eng.n_train
    t = {k: torch.from_numpy(a).cuda() for k, a in _optim_inputs(np.random.default_rng(0), n).items()}
    grad = torch.zeros(n + 4, dtype=torch.float32, device='cuda')
    regp = torch.zeros(2 + lib.hpe_optim_grid(n), dtype=torch.float32, device='cuda')
    ws = torch.zeros(int(c.prog.words[C.H_SLAB]), dtype=torch.float32, device='cuda')
    before = {k: v.clone() for k, v in t.items()}

    def optim(kind, it, m=None, n_=n):
        return lib.hpe_optim_step(kind, 1e-3, 0.9, 0.999, 1e-7, it, 1.0, ptr(t['w']), ptr(t['wt']),
                                  ptr(t['m']) if m is None else m, ptr(t['v']), ptr(grad), ptr(t['l2']),
                                  ptr(t['tpos']), n_, ptr(regp), _lib.stream())

    def fused(kind, it, m=None, n_=n):
        return lib.hpe_reduce_optim_step(c.h, 1, ptr(ws), ptr(grad), kind, 1e-3, 0.9, 0.999, 1e-7, it, 1.0,
                                         ptr(t['w']), ptr(t['wt']), ptr(t['m']) if m is None else m, ptr(t['v']),
                                         ptr(t['l2']), ptr(t['tpos']), n_, ptr(regp), _lib.stream())

    for fn, what in ((optim, 'hpe_optim_step'), (fused, 'hpe_reduce_optim_step')):
        for it in (0, -3):
            with pytest.raises(ValueError, match='iter must be >= 1'):
                _lib.check(fn(ADAM, it), what)
        with pytest.raises(ValueError, match='unknown optimizer kind 3'):
            _lib.check(fn(3, 1), what)
        with pytest.raises(ValueError, match='Adam/Adamax need m and v'):
            _lib.check(fn(ADAM, 1, m=NULL), what)
        with pytest.raises(ValueError, match='Adam/Adamax need m and v'):
            _lib.check(fn(ADAMAX, 1, m=NULL), what)
    with pytest.raises(ValueError, match='n = %d, the program trains %d parameters' % (n - 1, n)):
        _lib.check(fused(SGD, 1, n_=n - 1), 'hpe_reduce_optim_step')
    torch.cuda.synchronize()
    for k, v in t.items():
        assert torch.equal(v, before[k]), k
