"""Numpy emulator of the BlazeFace plan words (csrc/hpe_prog.h BFO_*) — TEST INFRASTRUCTURE.

Executes exactly what csrc/hpe_blaze.hip computes from the plan (padded channel strides, the stem's
6-row W^T table, depthwise tables, split head epilogue) in float64, so the plan builder's parameter
packing is checked against the oracle on CPU before the GPU runs the kernels.

``run(plan, images, dtype=np.float32)`` is the fp32 baseline of the same arithmetic.  ``hook``, when
given, is called as ``hook(i, f, name, arr)`` for every op record ``i`` (``f`` its words) with

    'x'     the op's input map, channels padded to cinp (blocks and heads) / the frame (stem)
    'xpad'  the zero-padded window source of the depthwise / stem conv
    'w'     the W^T table (coutp, cinp) of the 1x1 conv
    'd'     the 1x1 conv's A operand: the depthwise output (blocks) or the input map (heads)
    'res'   the residual added to the first cinp channels (identity or 2x2 max pool)
    'z'     the op's result before it is cut to its destination buffers (after the ReLU)

in this order; an array it returns replaces the one it was given (a test's mutants), ``None`` keeps
it.  A hook that only records sees every intermediate map and the operands an error bound needs.
``ops`` (record indices) runs only those records, on the buffers ``bufs`` of an earlier run: a test
continues one prefix of the graph with several different tails.
"""
import numpy as np

from hpe import blazeface as B


def _f(words, i):
    o = int(words[B.BFH_OPS_OFF]) + i * B.BFO_WORDS
    return [int(v) for v in words[o:o + B.BFO_WORDS]]


def stem_conv(xp, wt, Ho, Wo):
    """sum over the 6x5 window of the padded frame xp (n, 2Ho+6, 2Wo+5, 3) . wt (32, 6, 5, 3), stride 2"""
    y = np.zeros((xp.shape[0], Ho, Wo, 32), xp.dtype)
    for ky in range(6):
        for kx in range(5):
            win = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :]      # (n,Ho,Wo,3)
            y += win @ wt[:, ky, kx, :].T
    return y


def pad_window(xin, f):
    """the zero-padded map the 3x3 depthwise windows of op f read (TF 'same')"""
    H, W, Ho, Wo, s = f[B.BFO_H], f[B.BFO_W], f[B.BFO_HO], f[B.BFO_WO], f[B.BFO_STRIDE]
    pt, pl = f[B.BFO_PADT], f[B.BFO_PADL]
    xp = np.zeros((xin.shape[0], (Ho - 1) * s + 3, (Wo - 1) * s + 3, xin.shape[-1]), xin.dtype)
    hh = min(H, xp.shape[1] - pt)
    ww = min(W, xp.shape[2] - pl)
    xp[:, pt:pt + hh, pl:pl + ww] = xin[:, :hh, :ww]
    return xp


def depthwise(xp, tab, f):
    """tab[9] + the nine taps tab[0..8] (row-major) of the padded map, in the kernels' order"""
    Ho, Wo, s = f[B.BFO_HO], f[B.BFO_WO], f[B.BFO_STRIDE]
    a = np.broadcast_to(tab[9], (xp.shape[0], Ho, Wo, xp.shape[-1])).copy()
    for t in range(9):
        dy, dx = divmod(t, 3)
        a += xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s] * tab[t]
    return a


def run(plan, images, dtype=np.float64, hook=None, ops=None, bufs=None):
    words, P = plan['words'], plan['params'].astype(dtype)
    bufs = dict(bufs) if bufs is not None else {B.BUF_IMG: images.astype(dtype)}
    n = next(iter(bufs.values())).shape[0]

    def zeros(shape):
        return np.zeros(shape, dtype)

    for i in (range(int(words[B.BFH_NOPS])) if ops is None else ops):
        f = _f(words, i)
        if f[B.BFO_KIND] in (B.BF_STAGE, B.BF_FRONT):   # execution records: their ops follow as ordinary records
            continue

        def hk(name, arr, i=i, f=f):
            r = hook(i, f, name, arr) if hook is not None else None
            return arr if r is None else r

        x = bufs[f[B.BFO_SRC]]
        H, W, Ho, Wo = f[B.BFO_H], f[B.BFO_W], f[B.BFO_HO], f[B.BFO_WO]
        if f[B.BFO_KIND] == B.BF_STEM:
            wt = P[f[B.BFO_PWW]:f[B.BFO_PWW] + 32 * 90].reshape(32, 6, 5, 3)
            b = P[f[B.BFO_PWB]:f[B.BFO_PWB] + 32]
            pt, pl = f[B.BFO_PADT], f[B.BFO_PADL]
            x = hk('x', x)
            xp = zeros((n, 2 * Ho + 6, 2 * Wo + 5, 3))
            xp[:, pt:pt + H, pl:pl + W] = x
            xp = hk('xpad', xp)
            y = np.maximum(stem_conv(xp, wt, Ho, Wo) + b, 0)[..., :f[B.BFO_COUT]]
            bufs[f[B.BFO_DST]] = hk('z', y)
            continue
        cinp, cout, coutp = f[B.BFO_CINP], f[B.BFO_COUT], f[B.BFO_COUTP]
        xin = x.reshape(n, H, W, -1)
        if xin.shape[-1] < cinp:
            xin = np.concatenate([xin, zeros(xin.shape[:3] + (cinp - xin.shape[-1],))], -1)
        xin = hk('x', xin)
        if f[B.BFO_DW]:
            tab = P[f[B.BFO_DWW]:f[B.BFO_DWW] + 10 * cinp].reshape(10, cinp)
            a = depthwise(hk('xpad', pad_window(xin, f)), tab, f)
        else:
            a = xin
        wt = hk('w', P[f[B.BFO_PWW]:f[B.BFO_PWW] + coutp * cinp].reshape(coutp, cinp))
        a = hk('d', a)
        z = a @ wt.T + P[f[B.BFO_PWB]:f[B.BFO_PWB] + coutp]
        if f[B.BFO_RES] == B.RES_ID:
            z[..., :cinp] += hk('res', xin)
        elif f[B.BFO_RES] == B.RES_MAXPOOL:
            mp = np.maximum(np.maximum(xin[:, 0::2, 0::2], xin[:, 0::2, 1::2]),
                            np.maximum(xin[:, 1::2, 0::2], xin[:, 1::2, 1::2]))
            z[..., :cinp] += hk('res', mp)
        if f[B.BFO_RELU]:
            z = np.maximum(z, 0)
        z = hk('z', z)
        sp = f[B.BFO_SPLIT]
        if sp:
            bufs[f[B.BFO_DST]] = z[..., :sp]
            bufs[f[B.BFO_DST2]] = z[..., sp:cout]
        else:
            bufs[f[B.BFO_DST]] = z[..., :f[B.BFO_OSTRIDE]]
    return bufs
