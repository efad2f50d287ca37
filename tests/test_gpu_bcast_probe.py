"""The DPP row-broadcast operand on gfx950, through hpe_bcast_probe (csrc/hpe_rowprog.hip): the fused
regressor kernel's inline-asm helpers (csrc/hpe_dev.h fmac_bcast / mul_bcast: `v_fmac_f32_dpp` /
`v_mul_f32_dpp` with `row_newbcast:N row_mask:0xf bank_mask:0xf`) on one 64-lane wave, every N.

What the kernel relies on: lane l sees t[(l & ~15) + N] — lane N of its own 16-lane row — as the first
factor, in both instruction forms, for all sixteen N.  Inputs are small integers, so the products and
sums are exact in fp32 and the comparison is for equality."""
import ctypes

import numpy as np
import pytest

from hpe import _lib

pytestmark = pytest.mark.gpu

LANES = np.arange(64)


def _probe(t, x, acc):
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (t, x, acc)]
    out = torch.full((2, 16, 64), float('nan'), dtype=torch.float32, device='cuda')
    lib = _lib.load()
    _lib.check(lib.hpe_bcast_probe(*[ctypes.c_void_p(d.data_ptr()) for d in dev], ctypes.c_void_p(out.data_ptr()),
                                   None), 'hpe_bcast_probe')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bcast(t):
    """[16][64]: t[(lane & ~15) + N]."""
    return np.stack([t[(LANES & ~15) + n] for n in range(16)])


def test_broadcast_alone():
    """x = 1, acc = 0: both forms return the broadcast value itself, 64 distinct values."""
    t = (1000 + 7 * LANES).astype(np.float32)
    assert len(set(t)) == 64
    got = _probe(t, np.ones(64), np.zeros(64))
    want = _bcast(t)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)


def test_fmac_and_mul_forms():
    """Per-lane second factor and accumulator: only the first factor is broadcast."""
    rng = np.random.default_rng(3)
    t = rng.permutation(64).astype(np.float32) - 20
    x = rng.integers(-9, 10, 64).astype(np.float32)
    acc = rng.integers(-500, 500, 64).astype(np.float32)
    got = _probe(t, x, acc)
    b = _bcast(t)
    np.testing.assert_array_equal(got[0], b * x[None, :] + acc[None, :])
    np.testing.assert_array_equal(got[1], b * x[None, :])


def test_probe_rejects_null():
    assert _lib.load().hpe_bcast_probe(None, None, None, None, None) == 1
