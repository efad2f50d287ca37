"""Per-face regions of interest: hpe_preprocess_rois / hpe_face_rois (csrc/hpe_preproc.hip) and the
Python surface on top (hpe.preprocess.prepare_rois, BlazeFaceDetector.detect_rois / detect_refine,
FeatureExtractor(rois=)).

CPU: the restatement (tests/roi_ref.py: a numpy canvas handed whole to bicubic_ref.preprocess, the
ROI table in numpy float64) is pinned to what exists — an in-frame ROI is ``crop=``, an ROI reaching
outside is a padded frame — and to hand-made cases; argument checks need no device.
GPU: the kernels equal the restatement exactly (assert_array_equal throughout), and the entry points
built on them equal their parts composed by hand.

TF parity is unpinned as for the rest of frame preparation: the definition is bicubic_ref's restatement
applied to a padded canvas."""
import ctypes
import os

import numpy as np
import pytest

import bicubic_ref as B
import roi_ref as R
from hpe import _lib
from util import fixture

RID = 'reg1-stoqa9pt-reg2-hrchr82r-selected'
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')
FIELDS = ('boxes', 'keypoints', 'scores', 'poses')


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize('roi', [(3, 2, 9, 8), (0, 0, 19, 13), (5, 6, 1, 1), (4, 3, 3, 2)])
@pytest.mark.parametrize('bgr', [True, False])
def test_canvas_route_in_frame_is_crop(roi, bgr):
    u8 = _u8((2, 13, 19, 3), seed=1)
    got = R.prepare_rois(u8, [(1,) + roi, (0,) + roi], (13, 11), bgr=bgr, pad_value=(7, 130, 251))
    want = B.preprocess(u8, (13, 11), bgr=bgr, crop=roi)
    np.testing.assert_array_equal(got, want[[1, 0]])


@pytest.mark.parametrize('roi', [(-3, -2, 9, 8), (15, 9, 9, 8), (-5, -4, 30, 22), (1000, -1000, 7, 5)])
def test_canvas_route_outside_is_padded_frame(roi):
    """The frame padded on the host by more than the ROI sticks out, the ROI shifted by the padding."""
    u8 = _u8((1, 13, 19, 3), seed=2)
    pad = (7, 130, 251)
    x0, y0, w, h = roi
    if abs(x0) < 100:
        P = 12
        big = np.empty((1, 13 + 2 * P, 19 + 2 * P, 3), np.uint8)
        big[:] = np.uint8(pad)
        big[:, P:P + 13, P:P + 19] = u8
        want = B.preprocess(big, 8, crop=(x0 + P, y0 + P, w, h))
    else:                                            # no overlap: the canvas is all pad
        big = np.empty((1, h, w, 3), np.uint8)
        big[:] = np.uint8(pad)
        want = B.preprocess(big, 8)
    np.testing.assert_array_equal(R.prepare_rois(u8, [(0,) + roi], 8, pad_value=pad), want)


def test_canvas_pixels():
    f = _u8((4, 5, 3), seed=3)
    c = R.canvas(f, -1, 2, 4, 3, pad_value=(1, 2, 3))
    assert c.shape == (3, 4, 3)
    np.testing.assert_array_equal(c[:2, 1:], f[2:4, 0:3])
    assert (c[:, 0] == (1, 2, 3)).all() and (c[2] == (1, 2, 3)).all()
    assert (R.canvas(f, 0, 0, 5, 4) == f).all() and (R.canvas(f, 9, 0, 2, 2, 9) == 9).all()


def test_validity_rule():
    L = 1 << 24
    for roi in [(0, 0, 0, 1, 1), (2, -L, L, L, L), (1, L, -L, 1, 1)]:
        assert R.valid(roi, 3), roi
    for roi in [(-1, 0, 0, 1, 1), (3, 0, 0, 1, 1), (0, 0, 0, 0, 1), (0, 0, 0, 1, 0), (0, 0, 0, -4, 4),
                (0, 0, 0, L + 1, 1), (0, 0, 0, 1, L + 1), (0, L + 1, 0, 1, 1), (0, -L - 1, 0, 1, 1),
                (0, 0, L + 1, 1, 1), (0, 0, -L - 1, 1, 1), R.INVALID]:
        assert not R.valid(roi, 3), roi
    # the bounds keep every coordinate sum inside int32
    assert L + (L - 1) < 2 ** 31 and 3 * (L + L) < 2 ** 31
    # an invalid row's output is the prepared pad value, channel-swapped with bgr
    k = R.pad_constant(4, bgr=True, pad_value=(0, 51, 255))
    mid = (np.float32(51 / 255.0) - np.float32(0.5)) / np.float32(0.5)
    np.testing.assert_array_equal(k[0, 0], np.float32([1.0, mid, -1.0]))
    np.testing.assert_array_equal(R.pad_constant(4, bgr=False, pad_value=(0, 51, 255))[..., ::-1], k)
    u8 = _u8((1, 4, 4, 3), seed=4)
    np.testing.assert_array_equal(R.prepare_rois(u8, [(1, 0, 0, 2, 2)], 4, pad_value=(0, 51, 255))[0], k)


def _boxes(rows, M):
    """[[box, ...] per frame] -> count (n,), boxes (n, M, 4) float64 (unused slots: a poison value)."""
    n = len(rows)
    count = np.array([len(r) for r in rows], np.int32)
    boxes = np.full((n, M, 4), 1e300)
    for i, r in enumerate(rows):
        for j, b in enumerate(r):
            boxes[i, j] = b
    return count, boxes


HAND = [
    [(0.25, 0.25, 0.75, 0.5)],                        # inside: 48 x 24 px at (56, 24) .. (104, 48)
    [],
    [(-0.1, 0.4, 0.1, 0.6), (0.9, 0.4, 1.1, 0.6),     # crossing the left and the right border
     (0.4, -0.1, 0.6, 0.1), (0.4, 0.9, 0.6, 1.1)],    # the top and the bottom border
    [(np.nan, 0.1, 0.2, 0.3), (0.5, 0.5, 0.5, 0.5),   # NaN; zero size: S = 1
     (0.1, 0.1, np.inf, 0.2), (0.6, 0.7, 0.5, 0.6)],  # infinite; reversed corners: S = 1
    [],
]


def test_face_rois_twin_on_hand_made_boxes():
    count, boxes = _boxes(HAND, 4)
    src = (32, 0, 96, 96)
    rois, k = R.face_rois(count, boxes, src, 1.5)
    assert rois.shape == (20, 5) and rois.dtype == np.int32 and k == 9
    # 1.5 x 48 = 72 around the centre (80, 36)
    np.testing.assert_array_equal(rois[0], (0, 44, 0, 72, 72))
    # 0.2 x 96 = 19.2 (up to rounding) -> side 28.8 -> S = 29; centres 32 / 128 / 80 +- 14.5
    np.testing.assert_array_equal(rois[1:5], [(2, 17, 33, 29, 29), (2, 113, 33, 29, 29), (2, 65, -15, 29, 29),
                                              (2, 65, 81, 29, 29)])
    np.testing.assert_array_equal(rois[5], R.INVALID)
    np.testing.assert_array_equal(rois[6], (3, 79, 47, 1, 1))       # floor(80 - 0.5), floor(48 - 0.5)
    np.testing.assert_array_equal(rois[7], R.INVALID)
    np.testing.assert_array_equal(rois[8], (3, 84, 61, 1, 1))       # centre (84.8, 62.4)
    np.testing.assert_array_equal(rois[9:], np.tile(R.INVALID, (11, 1)))
    # the clamps: a huge finite box centred on the source's origin (32, 0) has S = 2^24 ...
    r2, k2 = R.face_rois(np.int32([1]), np.float64([[[-1e9, -1e9, 1e9, 1e9]]]), src, 2.0)
    assert k2 == 1
    np.testing.assert_array_equal(r2[0], (0, -(1 << 23) + 32, -(1 << 23), 1 << 24, 1 << 24))
    # ... and a far-away box has its origin at 2^24: still a valid (all pad) row
    r3, _ = R.face_rois(np.int32([1]), np.float64([[[1e9, 1e9, 1e9 + 1, 1e9 + 1]]]), src, 1.0)
    assert r3[0, 1] == 1 << 24 and r3[0, 2] == 1 << 24 and R.valid(r3[0], 1)
    # counts outside 0..max_faces are clamped
    assert R.face_rois(np.int32([9, -3]), np.zeros((2, 2, 4)), src, 1.0)[1] == 2
    # the remap inverts the ROI: the ROI's corners in the first pass's normalisation
    np.testing.assert_array_equal(R.remap([[0.0, 0.0], [1.0, 1.0]], rois[0], src),
                                  [[(44 - 32) / 96, 0.0], [(44 + 72 - 32) / 96, 72 / 96]])


# ---- interface, no device ----------------------------------------------------------------------

def test_signatures_are_bound():
    assert len(_lib.SIGNATURES['hpe_preprocess_rois'][1]) == 15
    assert len(_lib.SIGNATURES['hpe_face_rois'][1]) == 12
    assert _lib.SIGNATURES['hpe_face_rois'][1][8] is ctypes.c_double


@built
def test_hpe_preprocess_rois_rejects_bad_arguments():
    lib = _lib.load()
    z = ctypes.c_void_p(256)

    def call(frames=z, n=1, in_h=8, in_w=8, stride=24, rois=z, m=1, pad=(0, 0, 0), out=z, out_h=4, out_w=4):
        return lib.hpe_preprocess_rois(frames, n, in_h, in_w, stride, rois, m, pad[0], pad[1], pad[2], 1, out,
                                       out_h, out_w, None)

    assert call(frames=None) == 1
    assert b'hpe_preprocess_rois' in lib.hpe_last_error() and b'null' in lib.hpe_last_error()
    assert call(rois=None) == 1
    assert call(out=None) == 1
    assert call(n=-1) == 1
    assert call(m=-1) == 1
    assert b'negative' in lib.hpe_last_error()
    assert call(in_h=0) == 1
    assert call(in_w=0) == 1
    assert call(out_h=0) == 1
    assert call(out_w=-2) == 1
    assert call(stride=23) == 1
    assert b'stride' in lib.hpe_last_error()
    assert call(pad=(256, 0, 0)) == 1
    assert b'pad' in lib.hpe_last_error()
    assert call(pad=(0, -1, 0)) == 1
    assert call(pad=(0, 0, 1000)) == 1
    assert call(m=1 << 40, out_h=128, out_w=128) == 1   # m * out_h * out_w above INT32_MAX
    assert b'INT32_MAX' in lib.hpe_last_error()
    assert call(m=0) == 0
    assert call(frames=None, rois=None, out=None, m=0) == 0


@built
def test_hpe_face_rois_rejects_bad_arguments():
    lib = _lib.load()
    z = ctypes.c_void_p(256)

    def call(count=z, boxes=z, n=1, max_faces=4, src=(0, 0, 8, 8), scale=1.5, rois=z, n_rois=z):
        return lib.hpe_face_rois(count, boxes, n, max_faces, src[0], src[1], src[2], src[3], scale, rois, n_rois,
                                 None)

    assert call(count=None) == 1
    assert b'hpe_face_rois' in lib.hpe_last_error() and b'null' in lib.hpe_last_error()
    assert call(boxes=None) == 1
    assert call(rois=None) == 1
    assert call(n_rois=None) == 1
    assert call(n_rois=None, n=0) == 1
    assert call(n=-1) == 1
    assert call(max_faces=0) == 1
    assert b'max_faces' in lib.hpe_last_error()
    assert call(src=(0, 0, 0, 8)) == 1
    assert call(src=(0, 0, 8, -1)) == 1
    assert call(n=1 << 40, max_faces=100) == 1
    assert b'too large' in lib.hpe_last_error()


def test_prepare_rois_rejects_bad_frames_and_rois():
    import torch
    from hpe.preprocess import prepare_rois
    ok = np.zeros((8, 8, 3), np.uint8)
    for frames in (np.zeros((8, 8, 3), np.float32), torch.zeros((1, 8, 8, 3)), np.zeros((8, 8), np.uint8),
                   np.zeros((1, 1, 8, 8, 3), np.uint8), np.zeros((8, 8, 4), np.uint8)):
        with pytest.raises(ValueError):
            prepare_rois(frames, [(0, 0, 0, 4, 4)])
    for rois in ([(0, 0, 4, 4)], (0, 0, 0, 4, 4), np.zeros((2, 5, 1), np.int32), np.zeros((1, 5), np.float32),
                 torch.zeros((1, 5), dtype=torch.int64), torch.zeros((5,), dtype=torch.int32),
                 [(0, 0, 0, 4, 1 << 31)]):
        with pytest.raises(ValueError):
            prepare_rois(ok, rois)
    for pad in (256, -1, (1, 2), (1, 2, 3.5)):
        with pytest.raises(ValueError):
            prepare_rois(ok, [(0, 0, 0, 4, 4)], pad_value=pad)


def test_results_constructor_unchanged():
    from hpe.detector import Results
    r = Results(np.zeros((2, 4)), np.zeros((2, 6, 2)), np.zeros(2, np.float32), np.zeros((2, 3), np.float32))
    assert r.refined.dtype == bool and r.refined.shape == (2,) and not r.refined.any()


# ---- hpe_preprocess_rois -------------------------------------------------------------------------

PAD = (7, 130, 251)
L24 = 1 << 24
# (x0, y0, w, h) on a 13 x 19 frame
RECTS = [
    (3, 2, 9, 8),            # in frame
    (0, 0, 19, 13),          # the full frame
    (5, 6, 1, 1),            # one pixel
    (4, 3, 3, 2),            # 2 x 3: fewer than four source pixels
    (-3, -2, 9, 8),          # out at the top left: windows out in x only, in y only, in both
    (15, 9, 9, 8),           # out at the bottom right
    (-5, -4, 30, 22),        # the whole frame on a larger canvas
    (1000, -1000, 7, 5),     # all pad
    (L24, -L24, 5, 4),       # all pad, at the bounds of a valid row
]
IN_FRAME = 4


def _frames():
    wide = _u8((3, 13, 31, 3), seed=5)
    return wide, np.ascontiguousarray(wide[:, :, 4:23])


def _table():
    """Every rectangle on every frame, the frames in mixed order."""
    return np.array([((2 * i + f) % 3,) + r for f in range(3) for i, r in enumerate(RECTS)], np.int32)


def _gpu_rois(frames, rois, **kw):
    from hpe.preprocess import prepare_rois
    return prepare_rois(frames, rois, **kw).cpu().numpy()


def _gpu_input(frames, **kw):
    from hpe.preprocess import prepare_input
    return prepare_input(frames, **kw).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('size', [8, (13, 11), 128])
def test_gpu_rois_equal_prepare_input_and_canvas_route(size):
    import torch
    wide, u8 = _frames()
    view = torch.from_numpy(wide).cuda()[:, :, 4:23]
    assert not view.is_contiguous() and view.stride(1) == 31 * 3
    rois = _table()
    want = R.prepare_rois(u8, rois, size, pad_value=PAD)
    got = _gpu_rois(view, rois, size=size, pad_value=PAD)            # read in place through the row stride
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_gpu_rois(u8, rois, size=size, pad_value=PAD), want)   # contiguous host array
    np.testing.assert_array_equal(_gpu_rois(view, torch.from_numpy(rois).cuda(), size=size, pad_value=PAD), want)
    # against the existing kernel: crop= inside the frame, the host-built canvas as a whole frame otherwise
    for i, r in enumerate(RECTS):
        rows = [k for k in range(len(rois)) if k % len(RECTS) == i]
        if i < IN_FRAME:
            a = _gpu_input(view, size=size, crop=r)
            for k in rows:
                np.testing.assert_array_equal(got[k], a[rois[k, 0]])
        cv = np.stack([R.canvas(u8[rois[k, 0]], *r, pad_value=PAD) for k in rows])
        np.testing.assert_array_equal(got[rows], _gpu_input(cv, size=size))


@pytest.mark.gpu
@pytest.mark.parametrize('bgr', [True, False])
@pytest.mark.parametrize('pad', [0, PAD])
def test_gpu_rois_pad_value_and_channel_order(bgr, pad):
    _, u8 = _frames()
    rois = _table()
    got = _gpu_rois(u8, rois, size=(13, 11), bgr=bgr, pad_value=pad)
    np.testing.assert_array_equal(got, R.prepare_rois(u8, rois, (13, 11), bgr=bgr, pad_value=pad))
    # reversed bytes and pad with the other channel order give the same image
    p = pad if pad == 0 else pad[::-1]
    np.testing.assert_array_equal(_gpu_rois(np.ascontiguousarray(u8[..., ::-1]), rois, size=(13, 11), bgr=not bgr,
                                            pad_value=p), got)
    # a single (H, W, 3) frame
    one = rois[rois[:, 0] == 0]
    np.testing.assert_array_equal(_gpu_rois(u8[0], one, size=(13, 11), bgr=bgr, pad_value=pad), got[rois[:, 0] == 0])


@pytest.mark.gpu
def test_gpu_invalid_rows_give_the_pad_constant():
    import torch
    _, u8 = _frames()
    good = (1, 3, 2, 9, 8)
    bad = [(-1, 3, 2, 9, 8), (3, 3, 2, 9, 8), (1, 3, 2, 0, 8), (1, L24 + 1, 2, 9, 8), (1, 3, 2, 9, L24 + 1),
           (1, 3, -L24 - 1, 9, 8), (1, 3, 2, -9, 8), R.INVALID,
           (-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)]
    rois = np.array([x for b in bad for x in (good, b)] + [good], np.int64)
    for bgr in (True, False):
        out = torch.full((len(rois), 8, 8, 3), 77.0, device='cuda')
        from hpe.preprocess import prepare_rois
        assert prepare_rois(u8, rois, size=8, bgr=bgr, pad_value=PAD, out=out) is out
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got, R.prepare_rois(u8, rois, 8, bgr=bgr, pad_value=PAD))
        ref = B.preprocess(u8[1:2], 8, bgr=bgr, crop=good[1:])[0]
        k = R.pad_constant(8, bgr, PAD)
        for i in range(len(rois)):
            np.testing.assert_array_equal(got[i], ref if i % 2 == 0 else k)


@pytest.mark.gpu
def test_gpu_no_rois_and_no_frames():
    import torch
    _, u8 = _frames()
    got = _gpu_rois(u8, np.zeros((0, 5), np.int32), size=8)
    assert got.shape == (0, 8, 8, 3) and got.dtype == np.float32
    out = torch.full((0, 8, 8, 3), 1.0, device='cuda')
    assert _gpu_rois(u8, [], size=8, out=out).shape == (0, 8, 8, 3)
    # no frames: every row is invalid
    got = _gpu_rois(u8[:0], [(0, 0, 0, 4, 4)], size=4, pad_value=PAD)
    np.testing.assert_array_equal(got[0], R.pad_constant(4, True, PAD))


# ---- hpe_face_rois -------------------------------------------------------------------------------

def _gpu_face_rois(count, boxes, src, scale):
    import torch
    lib = _lib.load()
    n, M, _ = boxes.shape
    c = torch.from_numpy(np.ascontiguousarray(count, np.int32)).cuda()
    b = torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).cuda()
    rois = torch.full((n * M, 5), 12345, dtype=torch.int32, device='cuda')
    n_rois = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(lib.hpe_face_rois(p(c), p(b), n, M, src[0], src[1], src[2], src[3], scale, p(rois), p(n_rois), None),
               'hpe_face_rois')
    torch.cuda.synchronize()
    return rois.cpu().numpy(), int(n_rois.item())


@pytest.mark.gpu
def test_gpu_face_rois_hand_made():
    count, boxes = _boxes(HAND, 4)                   # frame 2 full (max_faces), frames 1 and 4 empty
    for src, scale in (((32, 0, 96, 96), 1.5), ((0, 0, 640, 480), 2.6), ((7, 3, 1, 1), 1.0)):
        want, k = R.face_rois(count, boxes, src, scale)
        got, gk = _gpu_face_rois(count, boxes, src, scale)
        assert gk == k == 9
        np.testing.assert_array_equal(got, want)
    huge = np.float64([[[-1e9, -1e9, 1e9, 1e9], [1e9, 1e9, 1e9 + 1, 1e9 + 1]]])
    want, k = R.face_rois(np.int32([2]), huge, (32, 0, 96, 96), 2.0)
    got, gk = _gpu_face_rois(np.int32([2]), huge, (32, 0, 96, 96), 2.0)
    assert gk == k == 2
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_gpu_face_rois_many_frames():
    """More frames than the workgroup has threads (the prefix over count strides), random boxes whose
    corners fall on both sides of every border, counts 0 .. max_faces and beyond."""
    rng = np.random.default_rng(6)
    n, M = 600, 3
    count = rng.integers(-1, M + 2, n).astype(np.int32)
    c = rng.uniform(-0.2, 1.2, (n, M, 2))
    half = rng.uniform(0, 0.3, (n, M, 2))
    boxes = np.concatenate([c - half, c + half], -1)
    boxes[rng.random((n, M)) < 0.05] = np.nan
    src = (80, 0, 480, 480)
    want, k = R.face_rois(count, boxes, src, 1.37)
    got, gk = _gpu_face_rois(count, boxes, src, 1.37)
    assert gk == k == int(np.clip(count, 0, M).sum()) and 0 < k < n * M
    np.testing.assert_array_equal(got, want)
    # no frames at all: n_rois is zeroed
    assert _gpu_face_rois(np.zeros(0, np.int32), np.zeros((0, M, 4)), src, 1.0)[1] == 0


# ---- end to end ----------------------------------------------------------------------------------

SCALE = 1.5
M_FACES = 8


@pytest.fixture(scope='module')
def e2e():
    """The first pass on the seeded noise frames, its ROI table by the numpy twin and the ROI images
    by the canvas route; computed once."""
    from hpe.detector import BlazeFaceDetector
    u8 = _u8((4, 96, 160, 3), seed=11)
    mc, w = fixture(RID)
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.15, max_faces=M_FACES)
    first = det.detect_images(u8, crop='square')
    src = B.crop_rect(96, 160, 'square')
    count = np.int32([len(r.scores) for r in first])
    boxes = np.zeros((4, M_FACES, 4))
    for i, r in enumerate(first):
        boxes[i, :count[i]] = r.boxes
    table, k = R.face_rois(count, boxes, src, SCALE)
    rois = table[:k]
    # not vacuous: a face in every frame, and an ROI sticking out of the top of the frame
    assert (count >= 1).all() and k == count.sum()
    assert (rois[:, 2] < 0).any()
    assert all(R.valid(r, 4) for r in rois)
    return dict(u8=u8, det=det, fixture=(mc, w), first=first, src=src, count=count, boxes=boxes, rois=rois,
                floats=R.prepare_rois(u8, rois, 128))


def _same(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, f
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_device_table_equals_twin(e2e):
    det = e2e['det']
    r = det.postprocess(det.net.forward(det.prepare(e2e['u8'], crop='square')))
    rois, n_rois = det.face_rois(r, e2e['src'], SCALE)
    m = int(n_rois.item())
    got = rois.cpu().numpy()
    assert m == len(e2e['rois']) and got.shape == (4 * M_FACES, 5)
    np.testing.assert_array_equal(got[:m], e2e['rois'])
    np.testing.assert_array_equal(got[m:], np.tile(R.INVALID, (4 * M_FACES - m, 1)))


@pytest.mark.gpu
def test_gpu_detect_rois_equals_detect_batch(e2e):
    det = e2e['det']
    a = det.detect_rois(e2e['u8'], e2e['rois'])
    b = det.detect_batch(e2e['floats'])
    assert len(a) == len(b) == len(e2e['rois'])
    for ra, rb in zip(a, b):
        _same(ra, rb)
    assert det.detect_rois(e2e['u8'], np.zeros((0, 5), np.int32)) == []


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [SCALE, 0.1])
def test_gpu_detect_refine_equals_its_parts(e2e, scale):
    """scale 1.5 is the issue's case; at 0.1 the ROIs are a few pixels of noise blown up to 128 x 128,
    to look at the faces the second pass does not replace as well (the count is printed either way)."""
    det, first, src = e2e['det'], e2e['first'], e2e['src']
    table, k = R.face_rois(e2e['count'], e2e['boxes'], src, scale)
    rois = table[:k]
    if scale == SCALE:
        np.testing.assert_array_equal(rois, e2e['rois'])
    second = det.detect_rois(e2e['u8'], rois)
    got = det.detect_refine(e2e['u8'], scale=scale, crop='square')
    assert len(got) == 4
    row = 0
    n_refined = 0
    for i in range(4):
        f = first[i]
        want = {k: getattr(f, k).copy() for k in FIELDS}
        refined = np.zeros(len(f.scores), bool)
        for j in range(len(f.scores)):
            s = second[row]
            if len(s.scores):
                want['scores'][j] = s.scores[0]
                want['poses'][j] = s.poses[0]
                want['boxes'][j] = R.remap(s.boxes[0].reshape(2, 2), rois[row], src).reshape(4)
                want['keypoints'][j] = R.remap(s.keypoints[0], rois[row], src)
                refined[j] = True
            row += 1
        for k in FIELDS:
            assert getattr(got[i], k).dtype == want[k].dtype
            np.testing.assert_array_equal(getattr(got[i], k), want[k])
        np.testing.assert_array_equal(got[i].refined, refined)
        n_refined += int(refined.sum())
    assert row == len(rois)
    print('detect_refine scale %g: %d of %d faces replaced by the second pass' % (scale, n_refined, row))


@pytest.mark.gpu
def test_gpu_detect_refine_without_faces(e2e):
    """A frame with no faces comes back as detect_images returns it (at a 0.9 threshold the noise
    frames have none: asserted, so the comparison is of empty results and not skipped)."""
    from hpe.detector import BlazeFaceDetector
    mc, w = e2e['fixture']
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.9, max_faces=M_FACES)
    b = det.detect_images(e2e['u8'], crop='square')
    assert all(len(r.scores) == 0 for r in b)
    a = det.detect_refine(e2e['u8'], scale=SCALE, crop='square')
    assert len(a) == 4
    for ra, rb in zip(a, b):
        _same(ra, rb)
        assert ra.refined.shape == (0,) and ra.refined.dtype == bool
    with pytest.raises(TypeError):
        det.detect_refine(e2e['u8'])                 # scale has no default


@pytest.mark.gpu
def test_gpu_feature_extractor_takes_rois(e2e, tmp_path):
    from hpe.features import FeatureExtractor
    mc, w = e2e['fixture']
    rois = e2e['rois']
    fe = FeatureExtractor(mc, w, scoreThreshold=0.15, max_faces=M_FACES)
    a = {k: v.cpu().numpy() for k, v in fe.extract_device(e2e['u8'], rois=rois).items()}
    b = {k: v.cpu().numpy() for k, v in fe.extract_device(e2e['floats']).items()}
    assert set(a) == set(b) and a['src'].shape == (len(rois), M_FACES)
    for k in ('count', 'src', 'feat88', 'feat96'):
        np.testing.assert_array_equal(a[k], b[k])
    for i in range(len(rois)):
        c = int(a['count'][i])
        for k in ('det_index', 'scores', 'boxes', 'keypoints', 'poses'):
            np.testing.assert_array_equal(a[k][i, :c], b[k][i, :c])
    # host arrays in slices of ROI rows, indexed by ROI row; the same rows reach build_datasets
    ea = fe.extract(e2e['u8'], batch_size=3, rois=rois)
    eb = fe.extract(e2e['floats'], batch_size=3)
    for x, y in zip(ea, eb):
        np.testing.assert_array_equal(x, y)
    poses = np.arange(12.0).reshape(4, 3)
    p0, p1 = fe.build_datasets(e2e['u8'], poses, str(tmp_path / 'roi'), batch_size=5, rois=rois)
    d0, d1 = np.load(p0), np.load(p1)
    np.testing.assert_array_equal(d0['features'], eb[0])
    np.testing.assert_array_equal(d1['features'], eb[2])
    np.testing.assert_array_equal(d0['poses'], poses[rois[eb[1], 0]])
    np.testing.assert_array_equal(d1['poses'], poses[rois[eb[3], 0]])
    with pytest.raises(ValueError):
        fe.extract_device(e2e['floats'], rois=rois)
    with pytest.raises(ValueError):
        fe.extract_device(e2e['u8'], rois=rois, crop='square')
