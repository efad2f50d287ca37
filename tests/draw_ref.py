"""numpy restatement of csrc/hpe_draw.hip (include/hpe.h states the rules): the three coverage rules,
the winner rule, the NV12 chroma rule, hpe_pose_prims and the colour conversion of hpe.draw.  Integer
arithmetic in int64 throughout; vectorised per primitive over its bounding box clipped to the frame."""
import math

import numpy as np

PRIM_WORDS, FACE_PRIMS, MAX_DIM, MAX_SIZE = 8, 11, 8192, 64
SENT = -123456789          # what the tests fill an output table with


def valid(row, n_colours):
    kind, x0, y0, x1, y1, size, colour = (int(v) for v in row[:7])
    return (kind in (1, 2, 3) and all(abs(c) <= MAX_DIM for c in (x0, y0, x1, y1))
            and (0 if kind == 2 else 1) <= size <= MAX_SIZE and 0 <= colour < n_colours)


def bbox(row):
    """The inclusive box outside which a valid row covers nothing."""
    kind, x0, y0, x1, y1, size = (int(v) for v in row[:6])
    if kind == 2:
        return x0 - size, y0 - size, x0 + size, y0 + size
    m = size // 2
    return min(x0, x1) - m, min(y0, y1) - m, max(x0, x1) + m, max(y0, y1) + m


def covers(row, X, Y):
    """The coverage rule of a valid row at the integer pixel arrays X, Y (int64) -> bool array."""
    kind, x0, y0, x1, y1, size = (int(v) for v in row[:6])
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if kind == 1:
        xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        h0, h1 = size // 2, (size - 1) // 2
        outer = (X >= xa - h0) & (X <= xb + h0) & (Y >= ya - h0) & (Y <= yb + h0)
        hole = (X >= xa + h1 + 1) & (X <= xb - h1 - 1) & (Y >= ya + h1 + 1) & (Y <= yb - h1 - 1)
        return outer & ~hole
    if kind == 2:
        return (X - x0) ** 2 + (Y - y0) ** 2 <= size * size
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    vx, vy = X - x0, Y - y0
    t = vx * dx + vy * dy
    th2 = size * size
    near0 = 4 * (vx * vx + vy * vy) <= th2
    near1 = 4 * ((X - x1) ** 2 + (Y - y1) ** 2) <= th2
    cross = vx * dy - vy * dx
    body = 4 * cross * cross <= th2 * L2
    return np.where(t <= 0, near0, np.where(t >= L2, near1, body))


def winners(h, w, prims, n_prims, n_colours):
    """One frame's table (P, 8) -> (h, w) int64: the index of the highest valid live row covering each
    pixel, -1 where none does."""
    P = len(prims)
    win = np.full((h, w), -1, np.int64)
    for i in range(min(max(int(n_prims), 0), P)):
        row = prims[i]
        if not valid(row, n_colours):
            continue
        bx0, by0, bx1, by1 = bbox(row)
        bx0, by0, bx1, by1 = max(bx0, 0), max(by0, 0), min(bx1, w - 1), min(by1, h - 1)
        if bx0 > bx1 or by0 > by1:
            continue
        Y, X = np.mgrid[by0:by1 + 1, bx0:bx1 + 1]
        c = covers(row, X, Y)
        sub = win[by0:by1 + 1, bx0:bx1 + 1]
        sub[c] = i
    return win


def draw(frames, prims, n_prims, colours):
    """frames (n, h, w, 3) uint8 (any strides), drawn in place as hpe_draw does."""
    n, h, w, _ = frames.shape
    colours = np.asarray(colours, np.uint8)
    for f in range(n):
        win = winners(h, w, prims[f], n_prims[f], len(colours))
        m = win >= 0
        col = np.asarray(prims[f])[win[m], 6]
        frames[f][m] = colours[col, :3]
    return frames


def draw_nv12(y, uv, prims, n_prims, colours):
    """y (n, h, w), uv (n, h / 2, w) uint8 (any strides), drawn in place as hpe_draw_nv12 does."""
    n, h, w = y.shape
    colours = np.asarray(colours, np.uint8)
    for f in range(n):
        win = winners(h, w, prims[f], n_prims[f], len(colours))
        col6 = np.asarray(prims[f])[:, 6]
        m = win >= 0
        y[f][m] = colours[col6[win[m]], 0]
        blk = win.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))       # the highest winning row of a block
        mb = blk >= 0
        c = colours[col6[blk[mb]]]
        by, bx = np.nonzero(mb)
        uv[f][by, 2 * bx] = c[:, 1]
        uv[f][by, 2 * bx + 1] = c[:, 2]
    return y, uv


# ---- hpe_pose_prims ------------------------------------------------------------------------------

def _clamp_dim(v):
    return min(max(int(v), -MAX_DIM), MAX_DIM)


def pix(v, s, o):
    with np.errstate(over='ignore'):
        t = math.trunc(min(max(float(np.trunc(np.float64(s) * np.float64(v))), -2.0 ** 30), 2.0 ** 30))
    return _clamp_dim(o + t)


def axis_values(x1, y1, x2, y2, pose):
    """The integer box corners and the (yaw, pitch, roll) float32 pose -> (cx, cy, the six untruncated
    endpoint values [Xx, Xy, Yx, Yy, Zx, Zy] as float64, tdx, tdy).  Python floats are IEEE doubles and
    every operation below rounds on its own."""
    yaw, pitch, roll = (float(np.float32(v)) for v in pose)
    tdx, tdy = (x1 + x2) / 2.0, (y1 + y2) / 2.0
    size = float(math.trunc(min(x2 - x1, y2 - y1) / 2.0))
    r, y, p = (-roll) / 180.0 * math.pi, (-yaw) / 180.0 * math.pi, (-pitch) / 180.0 * math.pi
    cr, sr, cy, sy, cp, sp = math.cos(r), math.sin(r), math.cos(y), math.sin(y), math.cos(p), math.sin(p)
    spsy = sp * sy
    m00 = cy * cr
    m10 = spsy * cr + cp * sr
    m01 = -(cy * sr)
    m11 = -(spsy * sr) + cp * cr
    m02 = sy
    m12 = -(sp * cy)
    vals = [m00 * size + tdx, -(m10 * size) + tdy, -(m01 * size) + tdx, m11 * size + tdy, m02 * size + tdx,
            -(m12 * size) + tdy]
    return math.trunc(tdx), math.trunc(tdy), vals, tdx, tdy


def pose_prims(count, boxes, keypoints, poses, src, sizes, prims=None):
    """hpe_pose_prims: -> (prims (n, 11 M, 8) int32, n_prims (n,) int32).  prims: the table to write into
    (rows at or past 11 c keep what they hold); None: a SENT-filled one."""
    n, M = boxes.shape[:2]
    x0, y0, sw, sh = (int(v) for v in src)
    box_th, kp_r, ath = int(sizes[0]), int(sizes[1]), [int(v) for v in sizes[2:5]]
    if prims is None:
        prims = np.full((n, FACE_PRIMS * M, PRIM_WORDS), SENT, np.int32)
    n_prims = np.zeros(n, np.int32)
    for i in range(n):
        c = min(max(int(count[i]), 0), M)
        n_prims[i] = FACE_PRIMS * c
        for j in range(c):
            rows = prims[i, FACE_PRIMS * j:FACE_PRIMS * (j + 1)]
            rows[:] = 0
            b = boxes[i, j]
            if not np.isfinite(b).all():
                continue
            x1, y1, x2, y2 = pix(b[0], sw, x0), pix(b[1], sh, y0), pix(b[2], sw, x0), pix(b[3], sh, y0)
            if box_th > 0:
                rows[0] = (1, x1, y1, x2, y2, box_th, 0, 0)
            for k in range(6):
                kx, ky = keypoints[i, j, k]
                if kp_r >= 0 and np.isfinite(kx) and np.isfinite(ky):
                    px, py = pix(kx, sw, x0), pix(ky, sh, y0)
                    rows[1 + k] = (2, px, py, px, py, kp_r, 1, 0)
            if np.isfinite(np.asarray(poses[i, j], np.float32)).all():
                cx, cy, v, _, _ = axis_values(x1, y1, x2, y2, poses[i, j])
                for k in range(3):
                    if ath[k] > 0:
                        rows[7 + k] = (3, cx, cy, _clamp_dim(math.trunc(v[2 * k])), _clamp_dim(math.trunc(v[2 * k + 1])),
                                       ath[k], 2 + k, 0)
    return prims, n_prims


# ---- the colour conversion of hpe.draw.bgr_to_yuv ------------------------------------------------

YUV = {'bt601': ((66, 129, 25), (-38, -74, 112), (112, -94, -18)),
       'bt709': ((47, 157, 16), (-26, -87, 112), (112, -102, -10))}


def bgr_to_yuv(bgr, matrix='bt601'):
    b, g, r = (int(c) for c in bgr)
    (a, o) = YUV[matrix], (16, 128, 128)
    return tuple(min(max(((m[0] * r + m[1] * g + m[2] * b + 128) >> 8) + k, 0), 255) for m, k in zip(a, o))
