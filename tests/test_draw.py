"""Detections and pose axes drawn into frames on the device: hpe_pose_prims, hpe_draw, hpe_draw_nv12
(csrc/hpe_draw.hip), hpe.draw and BlazeFaceDetector.draw / drawDetections on top.

CPU: the binding and the host-side argument checks; the restatement (tests/draw_ref.py) against a float64
distance test (segments) and against a literal transcription of the reference's geometry
(blazeFaceDetectorH5.py:186-206, :40-77); the margin of every geometry case from the one-ulp caveat of
include/hpe.h; the colour conversion.
GPU: the kernels equal the restatement bit for bit over whole allocations: frames are seeded random
bytes, so an unwritten pixel keeps its value, and the pitch padding, the gaps between frames and a
guard region after the last frame are compared too.

The rasteriser's tile is 128 x 8 pixels (DRAW_TW x DRAW_TH, one 2 x 2 block per thread of 256) and a
culling pass takes 256 rows into an LDS list of 256 (DRAW_LIST); the shapes below are chosen against
those numbers.  The fixtures hold no face images: the end-to-end tests cover the mechanism only, on
hand-made results.  Parity with OpenCV's rasterisation is not tested (no cv2); the coverage rules are
this project's."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

import draw_ref as D
import nv12_ref as N
from hpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')
TILE_W, TILE_H, LIST = 128, 8, 256
GUARD = 96
# 7 colours; byte 3 is set, and must be ignored
COLOURS = np.random.default_rng(5).integers(0, 256, (7, 4), dtype=np.uint8)


# ---- CPU: binding and host checks ----------------------------------------------------------------

def test_signatures_and_header():
    with open(os.path.join(ROOT, 'include', 'hpe.h')) as fh:
        src = fh.read()
    for name, nargs in (('hpe_draw', 12), ('hpe_draw_nv12', 15), ('hpe_pose_prims', 18)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r'^int %s\(([^;]*)\);' % name, src, re.M)
        assert m, name
        assert len(m.group(1).split(',')) == nargs
    for d in ('HPE_DRAW_PRIM_WORDS 8', 'HPE_DRAW_FACE_PRIMS 11', 'HPE_DRAW_MAX_DIM 8192', 'HPE_DRAW_MAX_SIZE 64'):
        assert '#define ' + d in src
    from hpe import draw
    assert (draw.PRIM_WORDS, draw.FACE_PRIMS, draw.MAX_DIM, draw.MAX_SIZE) == (
        D.PRIM_WORDS, D.FACE_PRIMS, D.MAX_DIM, D.MAX_SIZE) == (8, 11, 8192, 64)


def _draw_call(lib, p=1, **kw):
    """hpe_draw with valid scalars except ``kw``; every pointer is the dummy ``p`` (never dereferenced:
    the host checks come before any device call) or null."""
    a = dict(n=2, h=10, w=12, rs=36, fs=360, P=4, nc=5)
    a.update(kw)
    q = ctypes.c_void_p(p)
    return lib.hpe_draw(q, a['n'], a['h'], a['w'], a['rs'], a['fs'], q, q, a['P'], q, a['nc'], None)


def _nv12_call(lib, p=1, **kw):
    a = dict(n=2, h=10, w=12, yrs=12, yfs=120, uvrs=12, uvfs=60, P=4, nc=5)
    a.update(kw)
    q = ctypes.c_void_p(p)
    return lib.hpe_draw_nv12(q, q, a['n'], a['h'], a['w'], a['yrs'], a['yfs'], a['uvrs'], a['uvfs'], q, q, a['P'], q,
                             a['nc'], None)


def _pose_call(lib, p=1, **kw):
    a = dict(n=2, M=3, x0=0, y0=0, w=640, h=480, bt=2, kr=4, ax=3, ay=3, az=2)
    a.update(kw)
    q = ctypes.c_void_p(p)
    return lib.hpe_pose_prims(q, q, q, q, a['n'], a['M'], a['x0'], a['y0'], a['w'], a['h'], a['bt'], a['kr'], a['ax'],
                              a['ay'], a['az'], q, q, None)


@built
def test_c_abi_argument_checks_without_gpu():
    """Argument errors come back as HPE_EINVAL with a message naming the function, before any device
    call.  (Fails on a library without the three entry points.)"""
    lib = _lib.load()
    big = 1 << 62
    bad = [dict(n=-1), dict(P=-1), dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(h=-4), dict(rs=35),
           dict(rs=-36), dict(fs=-1), dict(nc=0), dict(nc=257), dict(nc=-1), dict(n=1 << 32), dict(n=1 << 31),
           dict(n=3, fs=big), dict(rs=big), dict(n=1 << 30, P=1 << 30), dict(n=1 << 24, h=8192, w=8192, rs=3 * 8192)]
    for kw in bad:
        assert _draw_call(lib, p=0, **kw) == 1, kw
        assert b'hpe_draw:' in lib.hpe_last_error(), kw
    assert _draw_call(lib, p=0) == 1 and b'hpe_draw: null' in lib.hpe_last_error()
    assert _draw_call(lib, p=0, n=0) == 0 and _draw_call(lib, p=0, P=0) == 0     # no-ops, also with null pointers
    assert _draw_call(lib, p=0, n=0, nc=0) == 1                                   # the scalars are still checked
    q, z = ctypes.c_void_p(1), ctypes.c_void_p(0)
    for i in range(4):
        f, pr, npr, col = [z if k == i else q for k in range(4)]
        assert lib.hpe_draw(f, 1, 4, 4, 12, 48, pr, npr, 1, col, 1, None) == 1, i

    bad = [dict(n=-1), dict(P=-1), dict(h=0), dict(w=0), dict(h=8194), dict(w=8194), dict(h=9), dict(w=11),
           dict(yrs=11), dict(uvrs=11), dict(yfs=-1), dict(uvfs=-1), dict(nc=0), dict(nc=257), dict(n=1 << 32),
           dict(n=3, yfs=big), dict(n=3, uvfs=big), dict(yrs=big), dict(uvrs=big), dict(n=1 << 30, P=1 << 30)]
    for kw in bad:
        assert _nv12_call(lib, p=0, **kw) == 1, kw
        assert b'hpe_draw_nv12:' in lib.hpe_last_error(), kw
    assert _nv12_call(lib, p=0) == 1 and b'hpe_draw_nv12: null' in lib.hpe_last_error()
    assert _nv12_call(lib, p=0, n=0) == 0 and _nv12_call(lib, p=0, P=0) == 0
    for i in range(5):
        y, uv, pr, npr, col = [z if k == i else q for k in range(5)]
        assert lib.hpe_draw_nv12(y, uv, 1, 4, 4, 4, 16, 4, 8, pr, npr, 1, col, 1, None) == 1, i

    lim = 1 << 24
    bad = [dict(n=-1), dict(M=0), dict(M=-1), dict(w=0), dict(h=0), dict(w=lim + 1), dict(h=lim + 1), dict(x0=lim + 1),
           dict(x0=-lim - 1), dict(y0=lim + 1), dict(y0=-lim - 1), dict(bt=-1), dict(bt=65), dict(ax=-1), dict(ax=65),
           dict(ay=-1), dict(ay=65), dict(az=-1), dict(az=65), dict(kr=-2), dict(kr=65),
           dict(n=1 << 20, M=1 << 10), dict(n=1 << 40, M=1)]
    for kw in bad:
        assert _pose_call(lib, p=0, **kw) == 1, kw
        assert b'hpe_pose_prims:' in lib.hpe_last_error(), kw
    assert _pose_call(lib, p=0) == 1 and b'hpe_pose_prims: null' in lib.hpe_last_error()
    assert _pose_call(lib, p=0, n=0) == 0
    assert _pose_call(lib, p=0, n=0, M=0) == 1
    for i in range(6):
        ptrs = [z if k == i else q for k in range(6)]
        assert lib.hpe_pose_prims(*ptrs[:4], 1, 1, 0, 0, 8, 8, 1, 1, 1, 1, 1, *ptrs[4:], None) == 1, i


def test_python_argument_errors_without_gpu():
    import torch
    from hpe import draw
    with pytest.raises(ValueError, match='in place'):
        draw.draw_prims(np.zeros((1, 4, 4, 3), np.uint8), torch.zeros((1, 1, 8), dtype=torch.int32),
                        torch.zeros(1, dtype=torch.int32), COLOURS)
    with pytest.raises(ValueError):
        draw.DrawStyle(box_colour=(1, 2, 300))
    with pytest.raises(ValueError):
        draw.bgr_to_yuv((1, 2, 3), 'bt2020')
    s = draw.DrawStyle(box=False, keypoints=False, axes=False)
    assert s.sizes() == (0, -1, 0, 0, 0) and draw.DrawStyle().sizes() == (2, 4, 3, 3, 2)
    t = draw.DrawStyle().colours()
    assert t.tolist() == [[22, 22, 250, 0], [214, 202, 18, 0], [0, 255, 0, 0], [0, 0, 255, 0], [255, 0, 0, 0]]
    assert draw.DrawStyle().colours(bgr=False)[:, :3].tolist() == t[:, 2::-1].tolist()


# ---- the tables of the rasteriser tests ----------------------------------------------------------

def _table(rows, P=None):
    """A list of (kind, x0, y0, x1, y1, size, colour) -> ((P, 8) int32, len(rows))."""
    P = max(len(rows), 1) if P is None else P
    t = np.zeros((P, 8), np.int32)
    for i, r in enumerate(rows):
        t[i, :7] = r
    return t, len(rows)


SEG_DIRS = [(0, 0), (25, 0), (-25, 0), (0, 12), (0, -12), (15, 15), (-15, 15), (15, -15), (-15, -15),
            (20, 3), (20, -3), (-20, 3), (-20, -3), (3, 20), (3, -20), (-3, 20), (-3, -20)]


def _kind_cases(w, h):
    """Each kind on its own at the limits: one table per case, centred in the frame."""
    cx, cy = w // 2, h // 2
    cases = []
    for th in (1, 2, 3, 64):
        cases.append([(1, cx - 20, cy - 6, cx + 21, cy + 5, th, 0)])
        cases.append([(1, cx + 21, cy + 5, cx - 20, cy - 6, th, 1)])        # flipped corners
        cases.append([(1, cx + 9, cy - 4, cx - 9, cy + 4, th, 2)])
        cases.append([(1, cx, cy, cx, cy, th, 3)])                          # too small to have a hole
        cases.append([(1, cx, cy, cx + 2, cy + 1, th, 4)])
    for r in (0, 1, 4, 64):
        cases.append([(2, cx, cy, -999, 999, r, 5)])                        # x1, y1 are ignored by a disk
    for th in (1, 2, 3, 64):
        for k, (dx, dy) in enumerate(SEG_DIRS):
            cases.append([(3, cx - dx // 2, cy - dy // 2, cx - dx // 2 + dx, cy - dy // 2 + dy, th, k % 7)])
    return cases


def _border_cases(w, h):
    """Primitives on tile borders, on the frame's edges, outside it, and at the coordinate limits."""
    c = [
        [(2, TILE_W, TILE_H, 0, 0, 4, 0)], [(2, TILE_W - 1, TILE_H - 1, 0, 0, 5, 1)],          # a tile corner
        [(1, TILE_W - 3, TILE_H - 2, TILE_W + 4, TILE_H + 3, 2, 2)],
        [(3, TILE_W - 20, TILE_H - 5, TILE_W + 9, TILE_H + 6, 3, 3)],
        [(3, 100, TILE_H - 1, 140, TILE_H - 1, 1, 4)], [(3, TILE_W - 1, 0, TILE_W - 1, h + 5, 1, 5)],  # last row / column
        [(3, 0, 2 * TILE_H - 1, w - 1, 2 * TILE_H - 1, 2, 6)], [(1, 0, 0, TILE_W - 1, TILE_H - 1, 1, 0)],
        [(1, TILE_W, TILE_H, w - 1, h - 1, 1, 1)], [(1, 0, 0, w - 1, h - 1, 3, 2)],
    ]
    for x, y in ((-2, 5), (w + 1, 5), (5, -2), (5, h + 1), (-3, -3), (w + 2, h + 2)):           # partly outside
        c.append([(2, x, y, 0, 0, 4, 3)])
        c.append([(1, x - 6, y - 3, x + 6, y + 3, 3, 4)])
        c.append([(3, x - 9, y - 4, x + 9, y + 4, 4, 5)])
    for x, y in ((-100, 5), (w + 100, 5), (5, -100), (5, h + 100), (-5, 5), (w + 4, 5), (5, -5), (5, h + 4)):
        c.append([(2, x, y, 0, 0, 4, 6), (3, x, y, x, y, 8, 0)])                                # wholly outside
    m = D.MAX_DIM
    c += [[(3, -m, -m, m, m, 3, 1)], [(3, -m, m, m, -m, 64, 2)], [(3, -m, 3, m, 5, 2, 3)], [(3, 7, -m, 9, m, 5, 4)],
          [(1, -m, -m, m, m, 64, 5)], [(1, -m, 3, m, 9, 2, 6)], [(2, -m, -m, m, m, 64, 0)], [(2, m, m, 0, 0, 64, 1)],
          [(3, m, m, -m, -m, 1, 2)], [(3, -m, 0, m, 1, 1, 3)], [(1, m, m, 5, 5, 1, 4)]]
    return c


def _order_cases(w, h):
    cx, cy = w // 2, h // 2
    three = [(1, cx - 12, cy - 5, cx + 12, cy + 5, 3, 0), (2, cx - 8, cy, 0, 0, 7, 1), (3, cx - 15, cy - 6, cx + 15, cy + 6, 4, 2)]
    cases = [list(p) for p in itertools.permutations(three)]
    cases.append([three[0], (0, 0, 0, 0, 0, 0, 0), three[1], (3, cx, cy, cx + 5, cy, 65, 3), three[2]])
    cases.append([three[2], (2, cx, cy, 0, 0, 64, 7), three[0]])            # colour == n_colours between them
    return cases


def _invalid_rows(w, h):
    cx, cy = w // 2, h // 2
    m = D.MAX_DIM
    return [(0, cx, cy, cx + 5, cy + 5, 3, 1), (4, cx, cy, cx + 5, cy + 5, 3, 1), (-1, cx, cy, cx + 5, cy + 5, 3, 1),
            (1, cx, cy, cx + 5, cy + 5, 0, 1), (3, cx, cy, cx + 5, cy + 5, 0, 1), (2, cx, cy, 0, 0, -1, 1),
            (1, cx, cy, cx + 5, cy + 5, 65, 1), (2, cx, cy, 0, 0, 65, 1), (3, cx, cy, cx + 5, cy + 5, 65, 1),
            (2, cx, cy, 0, 0, 3, -1), (2, cx, cy, 0, 0, 3, len(COLOURS)), (2, cx, cy, 0, 0, 3, 1 << 30),
            (2, cx, cy, m + 1, 0, 3, 1), (2, cx, cy, 0, -m - 1, 3, 1), (3, m + 1, cy, cx, cy, 3, 1),
            (3, cx, -m - 1, cx, cy, 3, 1), (1, -(1 << 31), cy, cx, cy, 3, 1), (3, cx, cy, (1 << 31) - 1, cy, 3, 1),
            (1 << 30, cx, cy, cx, cy, 3, 1), (2, cx, cy, 0, 0, -(1 << 31), 1)]


def _batch(cases):
    """Tables of different lengths -> (prims (n, P, 8), n_prims (n,)); the rows past a table's length hold
    a disk that would draw."""
    P = max(len(c) for c in cases) + 1
    prims = np.zeros((len(cases), P, 8), np.int32)
    prims[:, :, :7] = (2, 3, 3, 0, 0, 2, 1)
    n_prims = np.zeros(len(cases), np.int32)
    for i, c in enumerate(cases):
        prims[i, :len(c)] = _table(c)[0][:len(c)]
        n_prims[i] = len(c)
    return prims, n_prims


# ---- CPU: the restatement ------------------------------------------------------------------------

def test_ref_segment_rule_is_the_distance_to_the_segment():
    """Kind 3 equals a float64 test of the distance from the pixel centre to the segment against
    th / 2, on every pixel whose distance is not within 1e-9 of th / 2."""
    checked = 0
    for th in (1, 2, 3, 5, 64):
        for dx, dy in SEG_DIRS + [(8191, 3), (-4000, 8000)]:
            x0, y0 = 40 - dx // 2, 40 - dy // 2
            row = (3, x0, y0, x0 + dx, y0 + dy, th, 0, 0)
            Y, X = np.mgrid[-40:121, -40:121]
            got = D.covers(row, X, Y)
            vx, vy = (X - x0).astype(np.float64), (Y - y0).astype(np.float64)
            L2 = float(dx * dx + dy * dy)
            t = np.clip((vx * dx + vy * dy) / L2, 0.0, 1.0) if L2 else np.zeros_like(vx)
            dist = np.hypot(vx - t * dx, vy - t * dy)
            sure = np.abs(dist - th / 2.0) > 1e-9
            assert (got[sure] == (dist[sure] <= th / 2.0)).all(), (th, dx, dy)
            checked += int(sure.sum())
    assert checked > 2_000_000


def test_ref_rectangle_and_disk_by_hand():
    Y, X = np.mgrid[0:9, 0:9]
    g = D.covers((1, 2, 2, 6, 5, 1, 0, 0), X, Y)
    want = np.zeros((9, 9), bool)
    want[2:6, 2:7] = True
    want[3:5, 3:6] = False
    assert (g == want).all()
    g = D.covers((1, 6, 5, 2, 2, 2, 0, 0), X, Y)                # thickness 2: one pixel outward, none inward
    want = np.zeros((9, 9), bool)
    want[1:7, 1:8] = True
    want[3:5, 3:6] = False
    assert (g == want).all()
    assert D.covers((2, 4, 4, 0, 0, 0, 0, 0), X, Y).sum() == 1 and D.covers((2, 4, 4, 0, 0, 1, 0, 0), X, Y).sum() == 5
    assert D.covers((3, 4, 4, 4, 4, 1, 0, 0), X, Y).sum() == 1 and D.covers((3, 4, 4, 4, 4, 2, 0, 0), X, Y).sum() == 5


# ---- geometry cases (hpe_pose_prims), shared by the CPU and the GPU tests -------------------------

STYLE = (2, 4, 3, 3, 2)


def _faces(n, M, counts, seed, lo=0.05, hi=0.95):
    """Seeded detections: boxes of 5 .. 30 % of the source, keypoints inside them, angles N(0, 40)."""
    rng = np.random.default_rng(seed)
    d = dict(count=np.int32(counts), boxes=rng.uniform(lo, hi, (n, M, 4)), keypoints=rng.uniform(lo, hi, (n, M, 6, 2)),
             poses=rng.normal(0, 40, (n, M, 3)).astype(np.float32))
    s = rng.uniform(0.05, 0.3, (n, M, 2))
    d['boxes'][..., 2:] = d['boxes'][..., :2] + s
    return d


def _geometry_cases():
    """name -> (inputs, src, sizes)."""
    c = {}
    c['counts'] = (_faces(5, 4, [-1, 0, 1, 4, 7], 1), (0, 0, 1920, 1080), STYLE)
    c['offset'] = (_faces(3, 3, [3, 2, 3], 2), (37, -11, 640, 480), STYLE)
    c['outside'] = (_faces(2, 5, [5, 5], 3, lo=-0.6, hi=1.4), (0, 0, 300, 200), STYLE)
    d = _faces(2, 6, [6, 6], 4)
    d['boxes'][0, 0, 1] = np.nan
    d['boxes'][0, 1, 2] = np.inf
    d['keypoints'][0, 2, 3, 0] = np.nan
    d['keypoints'][0, 2, 5, 1] = -np.inf
    d['poses'][0, 3, 1] = np.nan
    d['poses'][0, 4, 2] = np.inf
    d['boxes'][1, 0] = (-1e300, 0.2, 1e300, 0.4)
    d['boxes'][1, 1] = (0.2, 1e300, 0.4, -1e300)
    d['boxes'][1, 2] = (1.7976931348623157e308, 0.1, 0.3, 0.2)
    d['keypoints'][1, 3, 0] = (1e300, -1e300)
    d['boxes'][1, 4] = (0.6, 0.7, 0.4, 0.3)                       # flipped: a negative size
    d['boxes'][1, 5] = (0.6, 0.3, 0.4, 0.5)                       # flipped in x only
    c['special'] = (d, (0, 0, 1920, 1080), STYLE)
    # angles of exactly 0 (and 90, 180): x1 + x2 and y1 + y2 odd, so the untruncated values are k + 0.5
    d = _faces(1, 4, [4], 5)
    d['boxes'][0, :] = (100.5 / 1920, 50.5 / 1080, 301.5 / 1920, 251.5 / 1080)
    d['poses'][0] = np.float32([[0, 0, 0], [0, 0, 30], [0, 25, 0], [15, 0, 0]])
    c['zero angles'] = (d, (0, 0, 1920, 1080), STYLE)
    for name, sizes in (('no box', (0, 4, 3, 3, 2)), ('no keypoints', (2, -1, 3, 3, 2)), ('no x', (2, 4, 0, 3, 2)),
                        ('no y', (2, 0, 3, 0, 2)), ('no z', (1, 64, 64, 64, 0)), ('nothing', (0, -1, 0, 0, 0))):
        c[name] = (_faces(2, 2, [2, 1], 6), (0, 0, 640, 480), sizes)
    c['e2e'] = (_e2e_results(), E2E_SRC, STYLE)
    return c


E2E_H, E2E_W, E2E_SRC = 90, 150, (30, 0, 90, 90)        # frames of 150 x 90, crop='square'


def _e2e_results():
    d = _faces(3, 4, [2, 0, 3], 7, lo=0.1, hi=0.6)
    d['scores'] = np.random.default_rng(8).uniform(0.5, 1, (3, 4)).astype(np.float32)
    return d


def _literal(box, pose, img_width, img_height, ox, oy):
    """blazeFaceDetectorH5.py:186-206 and :40-77 transcribed (numpy's astype(int), np.matmul, Python's
    int()), the angles as Python floats, the source rectangle's origin added to the pixel coordinates."""
    boundingBox = np.asarray(box, np.float64)
    x1 = ox + int((img_width * boundingBox[0]).astype(int))
    x2 = ox + int((img_width * boundingBox[2]).astype(int))
    y1 = oy + int((img_height * boundingBox[1]).astype(int))
    y2 = oy + int((img_height * boundingBox[3]).astype(int))
    yaw, pitch, roll = (float(v) for v in pose)
    tdx = (x1 + x2) / 2
    tdy = (y1 + y2) / 2
    size = int(min(x2 - x1, y2 - y1) / 2)

    def EulerToMatrix(roll, yaw, pitch):
        roll = roll / 180 * np.pi
        yaw = yaw / 180 * np.pi
        pitch = pitch / 180 * np.pi
        Rz = [[math.cos(roll), -math.sin(roll), 0], [math.sin(roll), math.cos(roll), 0], [0, 0, 1]]
        Ry = [[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]]
        Rx = [[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]]
        matrix = np.matmul(Rx, Ry)
        matrix = np.matmul(matrix, Rz)
        return matrix

    matrix = EulerToMatrix(-roll, -yaw, -pitch)
    Xaxis = np.array([matrix[0, 0], matrix[1, 0], matrix[2, 0]]) * size
    Yaxis = np.array([matrix[0, 1], matrix[1, 1], matrix[2, 1]]) * size
    Zaxis = np.array([matrix[0, 2], matrix[1, 2], matrix[2, 2]]) * size
    return (x1, y1, x2, y2), (int(tdx), int(tdy)), [(int(Xaxis[0] + tdx), int(-Xaxis[1] + tdy)),
                                                    (int(-Yaxis[0] + tdx), int(Yaxis[1] + tdy)),
                                                    (int(Zaxis[0] + tdx), int(-Zaxis[1] + tdy))]


def _live(d):
    M = d['boxes'].shape[1]
    for i in range(len(d['count'])):
        for j in range(min(max(int(d['count'][i]), 0), M)):
            yield i, j


def test_ref_geometry_equals_the_reference_transcribed():
    """The restatement's integer rows equal the literal transcription (np.matmul and all) on every
    geometry case whose values the transcription is defined for: finite, and small enough for
    astype(int) (the +-1e300 and 1.8e308 rows are clamped by rule and have no reference counterpart)."""
    seen = 0
    for name, (d, src, sizes) in _geometry_cases().items():
        prims, _ = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], src, STYLE)
        for i, j in _live(d):
            b, kp, po = d['boxes'][i, j], d['keypoints'][i, j], d['poses'][i, j]
            if not (np.isfinite(b).all() and np.abs(b).max() < 1e6 and np.isfinite(po).all()):
                continue
            rows = prims[i, 11 * j:11 * j + 11]
            corners, centre, ends = _literal(b, po, src[2], src[3], src[0], src[1])
            assert tuple(rows[0, :7]) == (1,) + corners + (2, 0), (name, i, j)
            for k in range(6):
                if np.isfinite(kp[k]).all() and np.abs(kp[k]).max() < 1e6:
                    x = src[0] + int((kp[k, 0] * src[2]).astype(int))
                    y = src[1] + int((kp[k, 1] * src[3]).astype(int))
                    assert tuple(rows[1 + k, :7]) == (2, x, y, x, y, 4, 1), (name, i, j, k)
            for k in range(3):
                assert tuple(rows[7 + k, :7]) == (3,) + centre + ends[k] + (STYLE[2 + k], 2 + k), (name, i, j, k)
            seen += 1
    assert seen >= 40


def test_geometry_cases_are_clear_of_the_one_ulp_caveat():
    """The device's sin / cos may differ from the host's by an ulp; at |size| <= 8192 that moves an
    untruncated endpoint value by about 1e-12 at the most.  Every such value of every geometry case is
    farther than 1e-6 from an integer, so the GPU tests below may demand the exact table."""
    n = 0
    for name, (d, src, sizes) in _geometry_cases().items():
        for i, j in _live(d):
            b, po = d['boxes'][i, j], d['poses'][i, j]
            if not (np.isfinite(b).all() and np.isfinite(po).all()):
                continue
            x1, y1, x2, y2 = (D.pix(b[0], src[2], src[0]), D.pix(b[1], src[3], src[1]), D.pix(b[2], src[2], src[0]),
                              D.pix(b[3], src[3], src[1]))
            _, _, vals, _, _ = D.axis_values(x1, y1, x2, y2, po)
            for v in vals:
                assert abs(v - round(v)) > 1e-6, (name, i, j, v)
                n += 1
    assert n >= 6 * 40
    d = _geometry_cases()['zero angles'][0]
    assert (d['poses'][0, 0] == 0).all()


def test_ref_omissions_and_non_finite():
    c = _geometry_cases()
    d, src, _ = c['special']
    p, n_prims = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], src, STYLE)
    assert n_prims.tolist() == [66, 66]
    assert (p[0, 0:22] == 0).all()                                    # NaN / inf in a box: all 11 rows
    assert (p[0, 22 + 4] == 0).all() and (p[0, 22 + 6] == 0).all() and p[0, 22 + 1, 0] == 2 and p[0, 22 + 7, 0] == 3
    assert (p[0, 33 + 7:33 + 10] == 0).all() and p[0, 33, 0] == 1 and (p[0, 33 + 1:33 + 7, 0] == 2).all()
    assert (p[0, 44 + 7:44 + 10] == 0).all()
    assert tuple(p[1, 0, 1:5]) == (-8192, 216, 8192, 432)             # +-1e300 clamps
    assert p[1, 44 + 7, 0] == 3 and p[1, 44, 1] > p[1, 44, 3]         # flipped box, drawn
    for name, rows in (('no box', [0]), ('no keypoints', range(1, 7)), ('no x', [7]), ('no y', [8]), ('no z', [9]),
                       ('nothing', range(11))):
        d, src, sizes = c[name]
        p, _ = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], src, sizes)
        for r in range(11):
            assert (p[0, r, 0] == 0) == (r in rows or r == 10), (name, r)     # row 10: reserved, zeros
    d, src, sizes = c['counts']
    p, n_prims = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], src, sizes)
    assert n_prims.tolist() == [0, 0, 11, 44, 44] and (p[2, 11:] == D.SENT).all() and (p[:2] == D.SENT).all()


def test_style_yuv_bytes_come_back_as_the_colour():
    """DrawStyle's (Y, U, V) bytes, put through the conversion hpe_preprocess_nv12 applies
    (tests/nv12_ref.py), come back within 3 levels per channel of the BGR colour.  Measured maximum over
    the five default colours: 1 level for bt601 and for bt709; over the 4096 colours of a grid of 16
    values per channel (steps of 17): 2 levels for bt601, 3 for bt709."""
    from hpe import draw
    style = draw.DrawStyle()
    for matrix in ('bt601', 'bt709'):
        yuv = style.colours(nv12=matrix)
        assert yuv.tolist() == [list(D.bgr_to_yuv(c, matrix)) + [0] for c in style.colours()[:, :3]]
        back = N.convert(yuv[:, 0], yuv[:, 1], yuv[:, 2], matrix).astype(int)
        err = np.abs(back - style.colours()[:, :3].astype(int)).max()
        print('default colours, %s: max error %d' % (matrix, err))
        assert err <= 3
    assert draw.bgr_to_yuv((255, 255, 255)) == (235, 128, 128) and draw.bgr_to_yuv((0, 0, 0)) == (16, 128, 128)


# ---- GPU: the rasteriser against the restatement -------------------------------------------------

def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _bytes_equal(got, want, what):
    bad = got != want
    assert not bad.any(), '%s: %d of %d bytes differ, first at offset %d' % (what, bad.sum(), bad.size,
                                                                           np.flatnonzero(bad)[0])


def _view(buf, off, shape, strides):
    return np.lib.stride_tricks.as_strided(buf[off:], shape, strides)


def _run_bgr(n, h, w, prims, n_prims, rs=None, gap=0, seed=0, colours=COLOURS):
    """hpe_draw on a seeded random allocation of n frames (row stride rs, ``gap`` bytes between frames,
    GUARD bytes after the last) and the restatement on a copy; the two allocations must be equal in
    every byte.  Returns (before, after)."""
    import torch
    rs = 3 * w if rs is None else rs
    fs = h * rs + gap
    size = (n - 1) * fs + h * rs + GUARD
    before = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    want = before.copy()
    D.draw(_view(want, 0, (n, h, w, 3), (fs, rs, 3, 1)), prims, n_prims, colours)
    dev = torch.from_numpy(before).cuda()
    tp = torch.from_numpy(np.ascontiguousarray(prims, np.int32)).cuda()
    tn = torch.from_numpy(np.ascontiguousarray(n_prims, np.int32)).cuda()
    tc = torch.from_numpy(np.ascontiguousarray(colours)).cuda()
    _lib.check(_lib.load().hpe_draw(_p(dev), n, h, w, rs, fs, _p(tp), _p(tn), prims.shape[1], _p(tc), len(colours),
                                    None), 'hpe_draw')
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    _bytes_equal(got, want, 'hpe_draw %dx%d' % (w, h))
    return before, got


def _run_nv12(n, h, w, prims, n_prims, pitch=None, gap=0, seed=0, packed=True, colours=COLOURS):
    """hpe_draw_nv12 likewise: the packed layout (uv = y + h * pitch within one allocation) or the two
    planes as separate allocations with pitches of their own.  Returns (before, after) per allocation."""
    import torch
    pitch = w if pitch is None else pitch
    rng = np.random.default_rng(seed)
    if packed:
        fs = (h + h // 2) * pitch + gap
        bufs = [rng.integers(0, 256, (n - 1) * fs + (h + h // 2) * pitch + GUARD, dtype=np.uint8)]
        lay = [(0, 0, pitch, fs), (0, h * pitch, pitch, fs)]             # (allocation, offset, row, frame)
    else:
        py, puv = pitch, pitch + 6
        fy, fuv = h * py + gap, (h // 2) * puv + 2 * gap
        bufs = [rng.integers(0, 256, (n - 1) * fy + h * py + GUARD, dtype=np.uint8),
                rng.integers(0, 256, (n - 1) * fuv + (h // 2) * puv + GUARD, dtype=np.uint8)]
        lay = [(0, 0, py, fy), (1, 0, puv, fuv)]
    want = [b.copy() for b in bufs]
    (ay, oy, ry, fy), (au, ou, ru, fu) = lay
    D.draw_nv12(_view(want[ay], oy, (n, h, w), (fy, ry, 1)), _view(want[au], ou, (n, h // 2, w), (fu, ru, 1)), prims,
                n_prims, colours)
    dev = [torch.from_numpy(b).cuda() for b in bufs]
    tp = torch.from_numpy(np.ascontiguousarray(prims, np.int32)).cuda()
    tn = torch.from_numpy(np.ascontiguousarray(n_prims, np.int32)).cuda()
    tc = torch.from_numpy(np.ascontiguousarray(colours)).cuda()
    _lib.check(_lib.load().hpe_draw_nv12(ctypes.c_void_p(dev[ay].data_ptr() + oy), ctypes.c_void_p(dev[au].data_ptr() + ou),
                                         n, h, w, ry, fy, ru, fu, _p(tp), _p(tn), prims.shape[1], _p(tc), len(colours),
                                         None), 'hpe_draw_nv12')
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in dev]
    for k, (g, x) in enumerate(zip(got, want)):
        _bytes_equal(g, x, 'hpe_draw_nv12 %dx%d allocation %d' % (w, h, k))
    return bufs, got


BGR_SIZES = [(141, 19), (70, 37), (1, 200), (200, 1), (128, 8), (129, 9)]      # (w, h); the tile is 128 x 8
NV12_SIZES = [(130, 18), (66, 34), (2, 2), (128, 8), (258, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize('w,h', BGR_SIZES)
def test_gpu_bgr_kinds_borders_and_order(w, h):
    """Every case is one frame of a batch with its own table, so each kind is drawn on its own; row
    stride above 3 w (and odd, so rows start at any byte address), a gap between the frames."""
    cases = _kind_cases(w, h) + _border_cases(w, h) + _order_cases(w, h)
    prims, n_prims = _batch(cases)
    before, after = _run_bgr(len(cases), h, w, prims, n_prims, rs=3 * w + 5, gap=11, seed=w)
    assert (before != after).any()


@pytest.mark.gpu
@pytest.mark.parametrize('w,h', NV12_SIZES)
@pytest.mark.parametrize('packed', [True, False])
def test_gpu_nv12_kinds_borders_and_order(w, h, packed):
    cases = _kind_cases(w, h) + _border_cases(w, h) + _order_cases(w, h)
    prims, n_prims = _batch(cases)
    before, after = _run_nv12(len(cases), h, w, prims, n_prims, pitch=w + 7, gap=13, seed=w, packed=packed)
    assert any((b != a).any() for b, a in zip(before, after))


@pytest.mark.gpu
def test_gpu_invalid_rows_draw_nothing():
    w, h = 141, 19
    cases = [[r] for r in _invalid_rows(w, h)]
    prims, n_prims = _batch(cases)
    prims[:, 1:] = 0                                  # nothing else in the tables
    n_prims[:] = prims.shape[1]
    before, after = _run_bgr(len(cases), h, w, prims, n_prims, rs=3 * w + 1, seed=1)
    _bytes_equal(after, before, 'invalid rows, packed')
    bufs, got = _run_nv12(len(cases), 18, 130, prims, n_prims, pitch=132, seed=2)
    _bytes_equal(got[0], bufs[0], 'invalid rows, NV12')
    # ... and a valid neighbour still draws, whatever stands beside it
    both = [[r, (2, w // 2, h // 2, 0, 0, 3, 2)] for r in _invalid_rows(w, h)] + \
           [[(2, w // 2, h // 2, 0, 0, 3, 2), r] for r in _invalid_rows(w, h)]
    prims, n_prims = _batch(both)
    before, after = _run_bgr(len(both), h, w, prims, n_prims, seed=3)
    assert (before != after).any()


@pytest.mark.gpu
def test_gpu_n_prims_bounds_the_live_rows():
    """n_prims of -3, 0, 1, P and P + 5; the rows past n_prims would draw and must not."""
    w, h, P = 141, 19, 6
    rows = [(2, 10 + 20 * i, 9, 0, 0, 6, i) for i in range(P)]
    counts = [-3, 0, 1, P - 1, P, P + 5, 1 << 30, -(1 << 31)]
    prims = np.stack([_table(rows)[0]] * len(counts))
    n_prims = np.int32(counts)
    before, after = _run_bgr(len(counts), h, w, prims, n_prims, gap=7, seed=4)
    fs = h * 3 * w + 7
    for k in (0, 1, 7):
        _bytes_equal(after[k * fs:(k + 1) * fs], before[k * fs:(k + 1) * fs], 'frame %d' % k)
    _run_nv12(len(counts), 18, 130, prims, n_prims, seed=5)


@pytest.mark.gpu
def test_gpu_more_survivors_than_one_culling_pass_holds():
    """2 * LIST + 1 small disks in one tile (three culling passes with the winner carried); the last one
    lies on the first and decides its pixels.  Also with the live rows ending inside a pass."""
    w, h = 141, 19
    n = 2 * LIST + 1
    rows = [(2, 3 + i % 120, 2 + (i // 120) % 4, 0, 0, 1, i % 7) for i in range(n - 1)] + [(2, 3, 2, 0, 0, 1, 6)]
    assert rows[0][6] != rows[-1][6]
    t, _ = _table(rows)
    prims = np.stack([t, t, t[::-1].copy()])
    n_prims = np.int32([n, LIST + 1, n])
    _run_bgr(3, h, w, prims, n_prims, rs=3 * w + 2, seed=6)
    _run_nv12(3, 18, 130, prims, n_prims, pitch=131, seed=7)
    win = D.winners(h, w, t, n, len(COLOURS))
    assert win[2, 3] == n - 1 and win[2, 4] == n - 1                     # the last row decides


@pytest.mark.gpu
def test_gpu_batch_frames_equal_frames_drawn_alone():
    """5 frames with different tables, an empty one among them: each frame of the batch is bit-equal
    to that frame drawn alone."""
    w, h = 141, 19
    cases = [_kind_cases(w, h)[0] + _border_cases(w, h)[3], [], _order_cases(w, h)[2], _kind_cases(w, h)[30],
             [(3, 0, 0, w, h, 5, 3), (1, 5, 2, 130, 15, 2, 4)]]
    prims, n_prims = _batch(cases)
    rs, gap = 3 * w + 3, 9
    fs = h * rs + gap
    before, after = _run_bgr(5, h, w, prims, n_prims, rs=rs, gap=gap, seed=8)
    for f in range(5):
        import torch
        one = torch.from_numpy(before[f * fs:f * fs + h * rs].copy()).cuda()
        tp, tn, tc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (prims[f:f + 1], n_prims[f:f + 1], COLOURS))
        _lib.check(_lib.load().hpe_draw(_p(one), 1, h, w, rs, 0, _p(tp), _p(tn), prims.shape[1], _p(tc), len(COLOURS),
                                        None), 'hpe_draw')
        _bytes_equal(one.cpu().numpy(), after[f * fs:f * fs + h * rs], 'frame %d alone' % f)
    _bytes_equal(after[fs:fs + h * rs], before[fs:fs + h * rs], 'the empty frame')
    _run_nv12(5, 18, 130, prims, n_prims, pitch=136, gap=5, seed=9, packed=False)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [True, False])
def test_gpu_nv12_chroma_rule(packed):
    """One-pixel-wide vertical lines on an odd and on an even column keep their colour; a block whose
    four pixels have four different winners takes the chroma of the highest row; a block with one
    pixel covered takes that row's chroma."""
    w, h = 66, 34
    cases = [[(3, 21, 3, 21, 30, 1, 0)], [(3, 20, 3, 20, 30, 1, 1)], [(3, 3, 11, 60, 11, 1, 2)], [(3, 3, 10, 60, 10, 1, 3)],
             [(2, 10, 10, 0, 0, 0, 0), (2, 11, 10, 0, 0, 0, 1), (2, 10, 11, 0, 0, 0, 2), (2, 11, 11, 0, 0, 0, 3)],
             [(2, 11, 11, 0, 0, 0, 3), (2, 10, 11, 0, 0, 0, 2), (2, 11, 10, 0, 0, 0, 1), (2, 10, 10, 0, 0, 0, 0)],
             [(2, 10, 11, 0, 0, 0, 2), (2, 11, 11, 0, 0, 0, 3), (2, 10, 10, 0, 0, 0, 0), (2, 11, 10, 0, 0, 0, 1)],
             [(2, 11, 11, 0, 0, 0, 4)], [(2, 10, 10, 0, 0, 0, 5)], [(2, 11, 10, 0, 0, 0, 6)], [(2, 10, 11, 0, 0, 0, 0)]]
    prims, n_prims = _batch(cases)
    bufs, got = _run_nv12(len(cases), h, w, prims, n_prims, pitch=w + 2, gap=3, seed=10, packed=packed)
    pitch = w + 2
    if packed:                                          # by hand, beside the restatement
        fs = (h + h // 2) * pitch + 3
        uv = _view(got[0], h * pitch, (len(cases), h // 2, w), (fs, pitch, 1))
        y = _view(got[0], 0, (len(cases), h, w), (fs, pitch, 1))
        assert (uv[0, 2:15, 20] == COLOURS[0, 1]).all() and (uv[0, 2:15, 21] == COLOURS[0, 2]).all()
        assert (y[0, 3:31, 21] == COLOURS[0, 0]).all()
        assert tuple(uv[4, 5, 10:12]) == tuple(COLOURS[3, 1:3]) and tuple(uv[5, 5, 10:12]) == tuple(COLOURS[0, 1:3])
        assert tuple(uv[6, 5, 10:12]) == tuple(COLOURS[1, 1:3]) and tuple(uv[7, 5, 10:12]) == tuple(COLOURS[4, 1:3])


# ---- GPU: hpe_pose_prims against the restatement -------------------------------------------------

def _gpu_pose_prims(d, src, sizes):
    import torch
    n, M = d['boxes'].shape[:2]
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('count', 'boxes', 'keypoints', 'poses')}
    assert t['count'].dtype == torch.int32 and t['boxes'].dtype == torch.float64 and t['poses'].dtype == torch.float32
    prims = torch.full((n, 11 * M, 8), D.SENT, dtype=torch.int32, device='cuda')
    n_prims = torch.full((n,), D.SENT, dtype=torch.int32, device='cuda')
    _lib.check(_lib.load().hpe_pose_prims(_p(t['count']), _p(t['boxes']), _p(t['keypoints']), _p(t['poses']), n, M,
                                          *src, *sizes, _p(prims), _p(n_prims), None), 'hpe_pose_prims')
    torch.cuda.synchronize()
    return prims.cpu().numpy(), n_prims.cpu().numpy()


@pytest.mark.gpu
def test_gpu_pose_prims_equals_the_restatement():
    """Every geometry case: the whole table, rows at or past 11 c still holding the sentinel, and
    n_prims, equal to the restatement.  (The cases are clear of the one-ulp caveat: the CPU test above.)"""
    for name, (d, src, sizes) in _geometry_cases().items():
        got, got_n = _gpu_pose_prims(d, src, sizes)
        want, want_n = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], src, sizes)
        bad = np.argwhere(got != want)
        assert not len(bad), '%s: %d words differ, first at %s: %s / %s' % (
            name, len(bad), bad[0], got[bad[0][0], bad[0][1]], want[bad[0][0], bad[0][1]])
        assert got_n.tolist() == want_n.tolist(), name
        for i in range(len(d['count'])):
            assert (got[i, int(want_n[i]):] == D.SENT).all(), (name, i)


# ---- GPU: end to end through Python (the mechanism only: hand-made results, no face images) -------

def _detector():
    import torch
    from hpe.detector import BlazeFaceDetector
    det = BlazeFaceDetector.__new__(BlazeFaceDetector)          # draw needs no network
    det.device = torch.device('cuda')
    det.max_faces = 4
    return det


def _host_list(d):
    from hpe.detector import Results
    return [Results(d['boxes'][i, :c], d['keypoints'][i, :c], d['scores'][i, :c], d['poses'][i, :c])
            for i, c in enumerate(int(c) for c in d['count'])]


def _e2e_want():
    d = _e2e_results()
    prims, n_prims = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], E2E_SRC, STYLE)
    prims[prims == D.SENT] = 0
    return prims, n_prims


@pytest.mark.gpu
def test_gpu_detector_draw_bgr():
    import torch
    from hpe import draw
    det, d = _detector(), _e2e_results()
    frames = np.random.default_rng(12).integers(0, 256, (3, E2E_H, E2E_W, 3), dtype=np.uint8)
    prims, n_prims = _e2e_want()
    want = D.draw(frames.copy(), prims, n_prims, draw.DrawStyle().colours())
    assert (want != frames).any() and (want[1] == frames[1]).all()
    # the device dict, a device tensor: in place, the same tensor back
    dev = torch.from_numpy(frames).cuda()
    r = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    out = det.draw(dev, r, crop='square')
    assert out is dev
    _bytes_equal(dev.cpu().numpy(), want, 'device dict')
    # the host Results list, a numpy input: left unchanged, a new array of the same kind
    keep = frames.copy()
    out = det.draw(frames, _host_list(d), crop='square')
    assert isinstance(out, np.ndarray) and out is not frames and (frames == keep).all()
    _bytes_equal(out, want, 'host list')
    # a pitched device view is written through its row stride; the padding stays
    big = torch.from_numpy(np.random.default_rng(13).integers(0, 256, (3, E2E_H, E2E_W + 9, 3), dtype=np.uint8)).cuda()
    pad = big[:, :, E2E_W:].clone()
    big[:, :, :E2E_W] = torch.from_numpy(frames).cuda()
    det.draw(big[:, :, :E2E_W], r, crop='square')
    _bytes_equal(big[:, :, :E2E_W].cpu().numpy(), want, 'pitched view')
    assert torch.equal(big[:, :, E2E_W:], pad)
    # RGB frames: bytes 0 and 2 of every colour swapped
    out = det.draw(frames, r, bgr=False, crop='square')
    _bytes_equal(out, D.draw(frames.copy(), prims, n_prims, draw.DrawStyle().colours(bgr=False)), 'rgb')
    # drawDetections: one host frame and its Results, into img
    one = frames[0, :, 30:120].copy()                              # the square itself: no crop needed
    img = one.copy()
    assert det.drawDetections(img, _host_list(d)[0]) is img
    _bytes_equal(img, det.draw(one, _host_list(d)[0]), 'drawDetections')
    _bytes_equal(img, want[0, :, 30:120], 'drawDetections against the cropped batch frame')
    # a style with parts switched off
    style = draw.DrawStyle(axes=False, box_thickness=1, keypoint_radius=2)
    p2, n2 = D.pose_prims(d['count'], d['boxes'], d['keypoints'], d['poses'], E2E_SRC, style.sizes())
    p2[p2 == D.SENT] = 0
    _bytes_equal(det.draw(frames, r, crop='square', style=style), D.draw(frames.copy(), p2, n2, style.colours()), 'style')


@pytest.mark.gpu
def test_gpu_detector_draw_nv12():
    import torch
    from hpe import draw
    from hpe.preprocess import NV12Frames
    det, d = _detector(), _e2e_results()
    rng = np.random.default_rng(14)
    y = rng.integers(0, 256, (3, E2E_H, E2E_W), dtype=np.uint8)
    uv = rng.integers(0, 256, (3, E2E_H // 2, E2E_W), dtype=np.uint8)
    prims, n_prims = _e2e_want()
    for matrix in ('bt601', 'bt709'):
        wy, wuv = D.draw_nv12(y.copy(), uv.copy(), prims, n_prims, draw.DrawStyle().colours(nv12=matrix))
        assert (wy != y).any() and (wuv != uv).any()
        out = det.draw(NV12Frames(y, uv, matrix), _host_list(d), crop='square')         # host in, host out
        assert isinstance(out, NV12Frames) and isinstance(out.y, np.ndarray) and out.matrix == matrix
        _bytes_equal(out.y, wy, 'y')
        _bytes_equal(out.uv, wuv, 'uv')
    # device planes, the packed layout: in place
    packed = torch.from_numpy(np.concatenate([y, uv], 1)).cuda()
    f = NV12Frames(packed, matrix='bt709')
    r = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    assert det.draw(f, r, crop='square') is f
    _bytes_equal(packed.cpu().numpy(), np.concatenate([wy, wuv], 1), 'packed device planes')
    with pytest.raises(ValueError, match='bgr'):
        det.draw(f, r, bgr=False)
