"""NV12 video frames in frame preparation and detection: hpe_preprocess_nv12 / hpe_preprocess_rois_nv12
(csrc/hpe_preproc.hip), hpe.preprocess.NV12Frames and everything that takes one.

The definition is tests/nv12_ref.py (the conversion of include/hpe.h in numpy int64) followed by the BGR
path that tests/test_preprocess.py and tests/test_rois.py pin, so every GPU comparison here is
assert_array_equal between a call on NV12 frames and the same call on nv12_to_bgr(frames).

CPU: the restatement over all 2^24 (Y, U, V) (within 1 of the float64 matrix, sums inside int32, the
range ends, the luma clamp), the chroma sample of a pixel, the bindings, every host-side argument
rejection of the two entry points, NV12Frames' validation.
OpenCV parity is unpinned: cv2 is not a dependency of the tests."""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libhpe.so is opened: the library then shares torch's HIP runtime)

import nv12_ref as N
import roi_ref as R
from hpe import _lib
from util import fixture

RID = 'reg1-stoqa9pt-reg2-hrchr82r-selected'
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')
MATRICES = ('bt601', 'bt709')
FIELDS = ('boxes', 'keypoints', 'scores', 'poses')


def _nv12(lead, h, w, seed):
    """Seeded planes: y lead + (h, w), uv lead + (h / 2, w / 2, 2)."""
    rng = np.random.default_rng(seed)
    lead = tuple(lead)
    return (rng.integers(0, 256, lead + (h, w), dtype=np.uint8),
            rng.integers(0, 256, lead + (h // 2, w // 2, 2), dtype=np.uint8))


# ---- the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize('matrix', MATRICES)
def test_conversion_over_all_inputs(matrix):
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    largest = 0
    differ = 0
    at16 = N.convert(np.full_like(U, 16), U, V, matrix)
    for Y in range(256):
        s = np.stack(N.sums(np.full_like(U, Y), U, V, matrix))
        largest = max(largest, int(np.abs(s).max()))
        got = N.convert(np.full_like(U, Y), U, V, matrix).astype(np.int64)
        want = N.convert_float(np.full_like(U, Y), U, V, matrix)
        assert np.abs(got - want).max() <= 1, Y
        differ += int((got != want).any(-1).sum())
        if Y < 16:
            np.testing.assert_array_equal(got, at16)
    assert largest < 2 ** 31
    print('%s: largest |sum| %.3e, %.4f %% of the inputs differ from the float64 matrix'
          % (matrix, largest, 100.0 * differ / 2 ** 24))
    assert differ < 0.05 * 2 ** 24
    np.testing.assert_array_equal(N.convert(16, 128, 128, matrix), (0, 0, 0))
    np.testing.assert_array_equal(N.convert(235, 128, 128, matrix), (255, 255, 255))


def test_tables_are_the_stated_constants():
    assert N.COEF['bt601'] == (1220542, 1673527, -852492, -409993, 2116026)
    assert N.COEF['bt709'] == tuple(int(np.floor(c * 2.0 ** 20 + 0.5)) for c in N.float_matrix('bt709'))
    assert N.COEF['bt709'] == (1220945, 1879825, -558796, -223607, 2215014)
    assert N.COEF['bt601'] == tuple(int(np.floor(c * 2.0 ** 20 + 0.5)) for c in N.float_matrix('bt601'))


def test_chroma_of_a_pixel_is_the_nearest_pair():
    """A chroma plane that is an index ramp: pixel (y, x) must carry pair (y >> 1, x >> 1)."""
    h, w = 6, 10
    y = np.random.default_rng(0).integers(0, 256, (h, w), dtype=np.uint8)
    idx = np.arange((h // 2) * (w // 2)).reshape(h // 2, w // 2)
    uv = np.stack([idx * 7 + 3, 250 - idx * 5], -1).astype(np.uint8)
    for matrix in MATRICES:
        bgr = N.nv12_to_bgr(y, uv, matrix)
        assert bgr.shape == (h, w, 3) and bgr.dtype == np.uint8
        for r in range(h):
            for c in range(w):
                u, v = uv[r >> 1, c >> 1]
                np.testing.assert_array_equal(bgr[r, c], N.convert(y[r, c], u, v, matrix))
        # both plane shapes, the packed layout and a batch axis
        np.testing.assert_array_equal(N.nv12_to_bgr(y, uv.reshape(h // 2, w), matrix), bgr)
        yy, cc = N.planes(np.concatenate([y, uv.reshape(h // 2, w)]))
        np.testing.assert_array_equal(N.nv12_to_bgr(yy, cc, matrix), bgr)
        np.testing.assert_array_equal(N.nv12_to_bgr(np.stack([y, y]), np.stack([uv, uv]), matrix)[1], bgr)


# ---- interface, no device ----------------------------------------------------------------------

def test_signatures_are_bound():
    a = _lib.SIGNATURES['hpe_preprocess_nv12'][1]
    b = _lib.SIGNATURES['hpe_preprocess_rois_nv12'][1]
    assert len(a) == 18 and len(b) == 19
    assert a[5:9] == [ctypes.c_int64] * 4 and b[5:9] == [ctypes.c_int64] * 4
    # the old entry points keep their signatures
    assert len(_lib.SIGNATURES['hpe_preprocess'][1]) == 14
    assert len(_lib.SIGNATURES['hpe_preprocess_rois'][1]) == 15


@built
def test_hpe_preprocess_nv12_rejects_bad_arguments():
    lib = _lib.load()
    z = ctypes.c_void_p(256)

    def call(y=z, uv=z, n=1, in_h=8, in_w=8, strides=(8, 64, 8, 32), matrix=0, crop=(0, 0, 8, 8), out=z, out_h=4,
             out_w=4):
        return lib.hpe_preprocess_nv12(y, uv, n, in_h, in_w, strides[0], strides[1], strides[2], strides[3], matrix,
                                       crop[0], crop[1], crop[2], crop[3], out, out_h, out_w, None)

    def refused(word, **kw):
        assert call(**kw) == 1, kw
        err = lib.hpe_last_error()
        assert b'hpe_preprocess_nv12' in err and b'hpe_preprocess_nv12_' not in err and word in err, (kw, err)

    refused(b'null', y=None)
    refused(b'null', uv=None)
    refused(b'null', out=None)
    refused(b'negative', n=-1)
    for kw in (dict(in_h=0), dict(in_w=0), dict(in_h=-8), dict(out_h=0), dict(out_w=-2), dict(crop=(0, 0, 0, 8)),
               dict(crop=(0, 0, 8, -1))):
        refused(b'positive', **kw)
    refused(b'even', in_h=7, crop=(0, 0, 4, 4))
    refused(b'even', in_w=9)
    refused(b'matrix', matrix=2)
    refused(b'matrix', matrix=-1)
    for crop in ((-1, 0, 4, 4), (0, -1, 4, 4), (5, 0, 4, 4), (0, 5, 4, 4), (0, 0, 9, 8), (2 ** 31 - 1, 0, 2, 2)):
        refused(b'crop', crop=crop)
    refused(b'stride', strides=(7, 64, 8, 32))
    refused(b'stride', strides=(8, 64, 7, 32))
    refused(b'stride', strides=(8, -1, 8, 32))
    refused(b'stride', strides=(8, 64, 8, -1))
    refused(b'too large', strides=(2 ** 62, 64, 8, 32))
    refused(b'too large', strides=(8, 64, 8, 2 ** 62), n=4)
    refused(b'INT32_MAX', n=1 << 40, out_h=128, out_w=128)
    assert call(n=0) == 0
    assert call(y=None, uv=None, out=None, n=0) == 0
    assert call(n=0, in_w=9) == 1                   # the frame description is checked even for no frames


@built
def test_hpe_preprocess_rois_nv12_rejects_bad_arguments():
    lib = _lib.load()
    z = ctypes.c_void_p(256)

    def call(y=z, uv=z, n=1, in_h=8, in_w=8, strides=(8, 64, 8, 32), rois=z, m=1, pad=(0, 0, 0), matrix=1, out=z,
             out_h=4, out_w=4):
        return lib.hpe_preprocess_rois_nv12(y, uv, n, in_h, in_w, strides[0], strides[1], strides[2], strides[3], rois,
                                            m, pad[0], pad[1], pad[2], matrix, out, out_h, out_w, None)

    def refused(word, **kw):
        assert call(**kw) == 1, kw
        err = lib.hpe_last_error()
        assert b'hpe_preprocess_rois_nv12' in err and word in err, (kw, err)

    refused(b'null', y=None)
    refused(b'null', uv=None)
    refused(b'null', rois=None)
    refused(b'null', out=None)
    refused(b'negative', n=-1)
    refused(b'negative', m=-1)
    for kw in (dict(in_h=0), dict(in_w=0), dict(out_h=0), dict(out_w=-2)):
        refused(b'positive', **kw)
    refused(b'even', in_h=7)
    refused(b'even', in_w=9)
    refused(b'matrix', matrix=2)
    refused(b'stride', strides=(7, 64, 8, 32))
    refused(b'stride', strides=(8, 64, 7, 32))
    refused(b'stride', strides=(8, -64, 8, 32))
    refused(b'too large', n=1 << 32)
    refused(b'too large', strides=(2 ** 62, 64, 8, 32))
    refused(b'pad', pad=(256, 0, 0))
    refused(b'pad', pad=(0, -1, 0))
    refused(b'pad', pad=(0, 0, 1000))
    refused(b'INT32_MAX', m=1 << 40, out_h=128, out_w=128)
    assert call(m=0) == 0
    assert call(y=None, uv=None, rois=None, out=None, m=0) == 0


def test_nv12frames_validation():
    import torch
    from hpe.preprocess import NV12Frames
    y, uv = _nv12((3,), 12, 20, seed=1)
    f = NV12Frames(y, uv)
    assert (f.n, f.h, f.w, f.matrix) == (3, 12, 20, 'bt601') and len(f) == 3
    assert (NV12Frames(y[0], uv[0]).n, NV12Frames(y[0], uv[0]).h) == (1, 12)
    g = NV12Frames(y, uv.reshape(3, 6, 20), 'bt709')[1:]
    assert isinstance(g, NV12Frames) and (g.n, g.h, g.w, g.matrix) == (2, 12, 20, 'bt709')
    np.testing.assert_array_equal(g.y, y[1:])
    np.testing.assert_array_equal(g.uv, uv[1:].reshape(2, 6, 20))
    assert NV12Frames(y[:0], uv[:0]).n == 0
    packed = np.concatenate([y, uv.reshape(3, 6, 20)], 1)
    p = NV12Frames(packed)
    assert (p.n, p.h, p.w) == (3, 12, 20)
    np.testing.assert_array_equal(p.y, y)
    np.testing.assert_array_equal(p.uv, uv.reshape(3, 6, 20))
    t = NV12Frames(torch.from_numpy(y), torch.from_numpy(uv))
    assert (t.n, t.h, t.w) == (3, 12, 20) and torch.is_tensor(t[:2].y) and t[:2].n == 2
    v = NV12Frames(*_nv12((2, 3), 4, 6, seed=2))                       # (S, T, H, W) for detect_video
    assert (v.n, len(v), v.lead, v.flat().lead) == (6, 2, (2, 3), (6,))
    for bad in (lambda: NV12Frames(y[:, :11], uv),                     # odd height
                lambda: NV12Frames(y[:, :, :19], uv),                  # odd width
                lambda: NV12Frames(y[:, :10], uv),                     # planes that do not belong together
                lambda: NV12Frames(y, uv[:2]),
                lambda: NV12Frames(y, uv[..., 0]),
                lambda: NV12Frames(y, uv[:, :, :, :1]),
                lambda: NV12Frames(y[0], uv),
                lambda: NV12Frames(y.astype(np.float32), uv),
                lambda: NV12Frames(y, uv.astype(np.int16)),
                lambda: NV12Frames(torch.zeros((12, 20)), torch.zeros((6, 20), dtype=torch.uint8)),
                lambda: NV12Frames(y, uv, matrix='bt2020'),
                lambda: NV12Frames(y, uv, matrix=0),
                lambda: NV12Frames(packed[:, :17]),                    # 17 rows are no 3H/2
                lambda: NV12Frames(packed[:, :, :19]),
                lambda: NV12Frames(np.zeros((20,), np.uint8)),
                lambda: NV12Frames(np.zeros((1, 1, 1, 12, 20), np.uint8), np.zeros((1, 1, 1, 6, 20), np.uint8))):
        with pytest.raises(ValueError):
            bad()
    assert NV12Frames(packed[:, :15]).h == 10                            # 15 rows of 20 are a 10 x 20 frame
    with pytest.raises(TypeError):
        f[0]


def test_bgr_false_and_plain_arrays():
    from hpe.detector import is_uint8
    from hpe.preprocess import NV12Frames, prepare_input, prepare_rois
    f = NV12Frames(*_nv12((2,), 12, 20, seed=3))
    assert is_uint8(f)
    with pytest.raises(ValueError, match='bgr'):
        prepare_input(f, bgr=False)
    with pytest.raises(ValueError, match='bgr'):
        prepare_rois(f, [(0, 0, 0, 4, 4)], bgr=False)
    with pytest.raises(ValueError):                                       # (S, T, H, W) is detect_video's alone
        prepare_input(NV12Frames(*_nv12((2, 2), 4, 6, seed=4)))
    with pytest.raises(ValueError):                                       # a 2-D uint8 array is still no frame
        prepare_input(np.zeros((12, 20), np.uint8))
    with pytest.raises(ValueError):
        prepare_rois(np.zeros((18, 20), np.uint8), [(0, 0, 0, 4, 4)])


def test_detector_methods_refuse_bgr_false():
    """Before any device work: the frames are checked first (no GPU is needed to get the ValueError)."""
    from hpe.detector import BlazeFaceDetector
    from hpe.preprocess import NV12Frames
    f = NV12Frames(*_nv12((2,), 12, 20, seed=3))
    det = BlazeFaceDetector.__new__(BlazeFaceDetector)                  # no network: the checks come first
    det.device = 'cpu'
    det.max_faces = 8
    with pytest.raises(ValueError, match='bgr'):
        det.detect_refine(f, 1.5, bgr=False)
    with pytest.raises(ValueError, match='bgr'):
        det.detect_tiled(f, 8, bgr=False)

    class Trk:
        streams = 1
    with pytest.raises(ValueError, match='bgr'):
        det.detect_video(f, Trk(), bgr=False)


# ---- hpe_preprocess_nv12 ---------------------------------------------------------------------------

def _gpu_input(frames, **kw):
    from hpe.preprocess import prepare_input
    return prepare_input(frames, **kw).cpu().numpy()


def _gpu_rois(frames, rois, **kw):
    from hpe.preprocess import prepare_rois
    return prepare_rois(frames, rois, **kw).cpu().numpy()


# on a 12 x 20 frame: every (x0, y0) parity, and a crop that ends at the frame's last row and column
CROPS = [None, 'square', (2, 2, 9, 8), (3, 2, 9, 8), (2, 3, 9, 8), (3, 3, 9, 8), (11, 4, 9, 8), (0, 0, 1, 1),
         (19, 11, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('size', [8, (13, 11), 128])
def test_gpu_crops_equal_the_bgr_path(size, matrix):
    from hpe.preprocess import NV12Frames
    y, uv = _nv12((3,), 12, 20, seed=5)
    bgr = N.nv12_to_bgr(y, uv, matrix)
    f = NV12Frames(y, uv, matrix)
    for crop in CROPS:
        got = _gpu_input(f, size=size, crop=crop)
        want = _gpu_input(bgr, size=size, crop=crop, bgr=True)
        assert got.dtype == np.float32 and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=str(crop))
    # one (H, W) frame
    np.testing.assert_array_equal(_gpu_input(NV12Frames(y[1], uv[1], matrix), size=size), _gpu_input(bgr[1], size=size))


# ---- hpe_preprocess_rois_nv12 ----------------------------------------------------------------------

PAD = (7, 130, 251)
L24 = 1 << 24
# (x0, y0, w, h)
ROIS = {
    (12, 20): [
        (2, 2, 9, 8), (3, 2, 9, 8), (2, 3, 9, 8), (3, 3, 9, 8),      # inside, every origin parity
        (0, 0, 20, 12),                                              # the whole frame
        (-3, 2, 9, 8), (15, 3, 9, 8), (4, -3, 9, 8), (5, 7, 9, 8),   # across the left, right, top, bottom border
        (-3, -2, 9, 8), (15, 9, 9, 8), (-4, 8, 9, 8), (14, -3, 9, 8),   # across the four corners
        (-5, -4, 30, 22),                                            # the whole frame on a larger canvas
        (1000, -1000, 7, 5), (L24, -L24, 5, 4),                      # entirely outside
        (5, 6, 1, 1), (6, 5, 1, 1), (19, 11, 1, 1), (-1, 0, 1, 1),   # one pixel
        (4, 3, 3, 2), (5, 4, 3, 2), (17, 10, 3, 2), (-1, -1, 3, 2),  # 3 x 2: taps clamp and repeat
    ],
    (64, 96): [
        (10, 10, 40, 40), (11, 10, 40, 40), (10, 11, 40, 40), (11, 11, 40, 40),
        (0, 0, 96, 64),
        (-7, 5, 30, 30), (80, 6, 30, 30), (20, -9, 30, 30), (21, 50, 30, 30),
        (-7, -9, 30, 30), (81, 51, 31, 29), (-8, 50, 30, 30), (79, -10, 30, 30),
        (-10, -10, 120, 90),
        (200, 200, 10, 10), (-L24, L24, 5, 4),
        (95, 63, 1, 1), (0, 0, 1, 1), (40, 33, 1, 1), (96, 10, 1, 1),
        (33, 21, 3, 2), (34, 22, 3, 2), (93, 62, 3, 2), (-2, 30, 3, 2),
    ],
}
INVALID = [(-1, 3, 2, 9, 8), (2, 3, 2, 9, 8), (1, 3, 2, 0, 8), (1, L24 + 1, 2, 9, 8), (1, 3, 2, 9, L24 + 1),
           (1, 3, -L24 - 1, 9, 8), (1, 3, 2, -9, 8), tuple(R.INVALID),
           (-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)]


def _table(hw):
    """Every rectangle on both frames, the frames in mixed order, an invalid row after every third."""
    rows = []
    for i, r in enumerate(ROIS[hw]):
        rows += [((i + f) % 2,) + r for f in range(2)]
        if i % 3 == 2:
            rows.append(INVALID[(i // 3) % len(INVALID)])
    return np.array(rows, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('pad', [0, PAD])
@pytest.mark.parametrize('size', [8, 16])         # 3 x 2 -> 16 x 16 is the upscale, 40 x 40 -> 8 x 8 the downscale
@pytest.mark.parametrize('hw', [(12, 20), (64, 96)])
def test_gpu_rois_equal_the_bgr_path(hw, size, pad, matrix):
    import torch
    from hpe.preprocess import NV12Frames
    y, uv = _nv12((2,), hw[0], hw[1], seed=6)
    bgr = N.nv12_to_bgr(y, uv, matrix)
    f = NV12Frames(y, uv, matrix)
    rois = _table(hw)
    bad = np.array([not R.valid(r, 2) for r in rois])
    assert bad.sum() == len(ROIS[hw]) // 3 and len(rois) == 2 * len(ROIS[hw]) + bad.sum()
    want = _gpu_rois(bgr, rois, size=size, pad_value=pad, bgr=True)
    out = torch.full((len(rois), size, size, 3), 77.0, device='cuda')
    from hpe.preprocess import prepare_rois
    assert prepare_rois(f, rois, size=size, pad_value=pad, out=out) is out
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    # an invalid row is the prepared pad constant (B, G, R bytes as they are, not converted)
    k = R.pad_constant(size, True, pad)
    for i in np.nonzero(bad)[0]:
        np.testing.assert_array_equal(got[i], k)
    # an ROI inside the frame is crop=
    for i in range(4):
        a = _gpu_input(f, size=size, crop=ROIS[hw][i])
        for j in (2 * i + i // 3, 2 * i + i // 3 + 1):
            assert tuple(rois[j, 1:]) == ROIS[hw][i]
            np.testing.assert_array_equal(got[j], a[rois[j, 0]])
    # the table on the device
    t = torch.from_numpy(rois.astype(np.int32)).cuda()
    np.testing.assert_array_equal(_gpu_rois(f, t, size=size, pad_value=pad), want)


@pytest.mark.gpu
def test_gpu_no_rois_and_no_frames():
    from hpe.preprocess import NV12Frames
    y, uv = _nv12((2,), 12, 20, seed=6)
    f = NV12Frames(y, uv)
    got = _gpu_rois(f, np.zeros((0, 5), np.int32), size=8)
    assert got.shape == (0, 8, 8, 3) and got.dtype == np.float32
    # no frames: every row is invalid
    got = _gpu_rois(f[:0], [(0, 0, 0, 4, 4)], size=4, pad_value=PAD)
    np.testing.assert_array_equal(got[0], R.pad_constant(4, True, PAD))
    got = _gpu_input(f[:0], size=8)
    assert got.shape == (0, 8, 8, 3) and got.dtype == np.float32


# ---- both sources, crop and ROI form: every rectangle of a tiny frame -----------------------------------

TINY = (4, 6)                         # rows x columns: every window is an edge case
TINY_SIZES = [(5, 3), (1, 1)]


def _tiny_inside():
    """Every rectangle (x0, y0, w, h) inside the tiny frame."""
    H, W = TINY
    return [(x0, y0, w, h) for y0 in range(H) for h in range(1, H - y0 + 1) for x0 in range(W)
            for w in range(1, W - x0 + 1)]


def _tiny_outside():
    """Every rectangle with sides 1..5 and an origin from -4 to one past the far edge that reaches outside."""
    H, W = TINY
    return [(x0, y0, w, h) for h in range(1, 6) for w in range(1, 6) for y0 in range(-4, H + 2)
            for x0 in range(-4, W + 2) if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H]


def test_tiny_rectangles_are_what_they_claim():
    inside, outside = _tiny_inside(), _tiny_outside()
    assert len(inside) == 210 and len(set(inside)) == 210 and not set(inside) & set(outside)
    assert len(inside) + len(outside) == 25 * 10 * 12 + sum(1 for r in inside if r[2] > 5)
    for axis, far in ((0, TINY[1]), (1, TINY[0])):
        assert {r[axis] for r in outside} == set(range(-4, far + 2))       # odd and even origins, past the far edge
        assert {r[2 + axis] for r in outside} == set(range(1, 6))


@pytest.mark.gpu
def test_gpu_every_rectangle_of_a_tiny_frame():
    """The four specializations share their branch structure: each rectangle inside the frame through the
    crop form and as a row of one ROI table, the rectangles reaching outside as a second table, both
    sources, all equal to the numpy restatement (and crop == ROI) bit for bit."""
    import torch
    import bicubic_ref as B
    from hpe.preprocess import NV12Frames, prepare_input, prepare_rois
    y, uv = _nv12((1,), TINY[0], TINY[1], seed=12)
    bgr = N.nv12_to_bgr(y, uv)
    sources = {'bgr': torch.from_numpy(bgr).cuda(),
               'nv12': NV12Frames(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())}
    inside, outside = _tiny_inside(), _tiny_outside()
    t_in = torch.tensor([(0,) + r for r in inside], dtype=torch.int32).cuda()
    t_out = np.array([(0,) + r for r in outside], np.int32)
    for size in TINY_SIZES:
        want_in = np.stack([B.preprocess(bgr, size, crop=r)[0] for r in inside])
        want_out = R.prepare_rois(bgr, t_out, size, pad_value=PAD)
        for name, f in sources.items():
            crops = torch.cat([prepare_input(f, size=size, crop=r) for r in inside]).cpu().numpy()
            rois = prepare_rois(f, t_in, size=size, pad_value=PAD).cpu().numpy()
            for i, r in enumerate(inside):
                where = '%s %s crop %s' % (name, size, r)
                np.testing.assert_array_equal(crops[i], want_in[i], err_msg=where)
                np.testing.assert_array_equal(rois[i], want_in[i], err_msg=where + ' as an ROI')
            np.testing.assert_array_equal(crops, rois)
            got = prepare_rois(f, t_out, size=size, pad_value=PAD).cpu().numpy()
            for i, r in enumerate(outside):
                np.testing.assert_array_equal(got[i], want_out[i], err_msg='%s %s ROI %s' % (name, size, r))


# ---- the conversion itself, through an identity resize -----------------------------------------------

Y16 = [0, 1, 15, 16, 17, 64, 128, 180, 234, 235, 236, 254, 255]


def _prepared(bgr):
    """What frame preparation makes of BGR bytes when the resize is the identity: the / 255 table of
    the byte, (x - 0.5) / 0.5, RGB."""
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    return (lut[bgr[..., ::-1]] - np.float32(0.5)) / np.float32(0.5)


def _all_pairs_frames():
    """Four 512 x 512 frames whose chroma plane holds every (U, V) pair; the four luma samples of a pair
    and the four frames carry 16 Y values."""
    rng = np.random.default_rng(7)
    ys = np.array(Y16 + [int(v) for v in rng.integers(0, 256, 3)], np.uint8).reshape(4, 2, 2)
    r, c = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    uv = np.stack([np.stack([(c + 37 * f) & 255, (r + 91 * f) & 255], -1) for f in range(4)]).astype(np.uint8)
    y = np.stack([np.tile(ys[f], (256, 256)) for f in range(4)])
    for f in range(4):
        assert len(set(map(tuple, uv[f].reshape(-1, 2).tolist()))) == 65536
    return y, uv


def _all_luma_frame():
    """One frame with every Y in 0..255 at 1,024 seeded (U, V) pairs and the nine pairs of {0, 128,
    255}^2: chroma row p holds pair p in all its 64 columns, and the 2 x 128 luma samples above it
    are a permutation of 0..255."""
    rng = np.random.default_rng(8)
    pairs = np.concatenate([rng.integers(0, 256, (1024, 2)), [(u, v) for u in (0, 128, 255) for v in (0, 128, 255)]])
    pairs = np.concatenate([pairs, pairs[:1]])[:1034 // 2 * 2]          # an even count keeps it simple
    p = len(pairs)
    uv = np.repeat(pairs[:, None, :], 64, axis=1).astype(np.uint8)      # (p, 64, 2)
    dy, x = np.meshgrid(np.arange(2), np.arange(128), indexing='ij')
    y = np.stack([(2 * x + dy + 17 * i) & 255 for i in range(p)]).reshape(2 * p, 128).astype(np.uint8)
    assert sorted(y[:2].ravel().tolist()) == list(range(256))
    return y[None], uv[None]


@pytest.mark.gpu
@pytest.mark.parametrize('matrix', MATRICES)
def test_gpu_conversion_through_an_identity_resize(matrix):
    from hpe.preprocess import NV12Frames
    for y, uv in (_all_pairs_frames(), _all_luma_frame()):
        h, w = y.shape[-2:]
        bgr = N.nv12_to_bgr(y, uv, matrix)
        got = _gpu_input(NV12Frames(y, uv, matrix), size=(h, w))
        np.testing.assert_array_equal(got, _gpu_input(bgr, size=(h, w), bgr=True))
        np.testing.assert_array_equal(got, _prepared(bgr))
        # and as one ROI per frame
        rois = [(i, 0, 0, w, h) for i in range(len(y))]
        np.testing.assert_array_equal(_gpu_rois(NV12Frames(y, uv, matrix), rois, size=(h, w)), got)


# ---- layouts -------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_layouts():
    import torch
    from hpe.preprocess import NV12Frames, _device_frames
    n, h, w = 3, 12, 20
    y, uv = _nv12((n,), h, w, seed=9)
    rois = _table((h, w))
    rois = rois[rois[:, 0] < 2]
    want = _gpu_input(NV12Frames(y, uv), size=(13, 11), crop=(3, 2, 15, 9))
    want_r = _gpu_rois(NV12Frames(y, uv), rois, size=8, pad_value=PAD)
    np.testing.assert_array_equal(want, _gpu_input(N.nv12_to_bgr(y, uv), size=(13, 11), crop=(3, 2, 15, 9)))

    def same(f, in_place):
        d,(sy, fy, suv, fuv) = _device_frames(f, None, None, 'test')
        for plane, src in ((d.y, f.y), (d.uv, f.uv)):
            if in_place:
                assert torch.is_tensor(src) and plane.data_ptr() == src.data_ptr()
        np.testing.assert_array_equal(_gpu_input(f, size=(13, 11), crop=(3, 2, 15, 9)), want)
        np.testing.assert_array_equal(_gpu_rois(f, rois, size=8, pad_value=PAD), want_r)
        return sy, fy, suv, fuv

    # host numpy: two planes (both uv shapes), packed
    same(NV12Frames(y, uv.reshape(n, h // 2, w)), False)
    packed = np.concatenate([y, uv.reshape(n, h // 2, w)], 1)
    same(NV12Frames(packed), False)
    # device tensors, contiguous, and the packed layout read in place: uv = y + H * pitch
    same(NV12Frames(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()), True)
    tp = torch.from_numpy(packed).cuda()
    assert same(NV12Frames(tp), True) == (w, 3 * h // 2 * w, w, 3 * h // 2 * w)
    # a pitch above W: slices of wider tensors whose spare columns hold seeded bytes
    rng = np.random.default_rng(10)
    wide = rng.integers(0, 256, (n, 3 * h // 2, 37), dtype=np.uint8)
    wide[:, :, 5:5 + w] = packed
    tw = torch.from_numpy(wide).cuda()
    view = tw[:, :, 5:5 + w]
    assert not view.is_contiguous()
    assert same(NV12Frames(view), True) == (37, 3 * h // 2 * 37, 37, 3 * h // 2 * 37)
    # a uv plane of its own: another pitch, spare rows between the frames, the (n, H/2, W/2, 2) shape
    cw = rng.integers(0, 256, (n, h // 2 + 3, 26, 2), dtype=np.uint8)
    cw[:, 1:1 + h // 2, 2:2 + w // 2] = uv
    tc = torch.from_numpy(cw).cuda()[:, 1:1 + h // 2, 2:2 + w // 2]
    ty = tw[:, :h, 5:5 + w]
    assert same(NV12Frames(ty, tc), True) == (37, 3 * h // 2 * 37, 52, (h // 2 + 3) * 52)
    # rows that are not contiguous are copied
    yt = torch.from_numpy(np.ascontiguousarray(y.transpose(0, 2, 1))).cuda().transpose(1, 2)
    same(NV12Frames(yt, torch.from_numpy(uv).cuda()), False)
    # one plane on the host, one on the device
    same(NV12Frames(y, torch.from_numpy(uv).cuda()), False)


# ---- the detector's methods ----------------------------------------------------------------------

M_FACES = 8
SCALE = 1.5


@pytest.fixture(scope='module')
def e2e():
    """Seeded NV12 noise frames, their BGR conversion and a detector on the committed unified graph."""
    from hpe.detector import BlazeFaceDetector
    from hpe.preprocess import NV12Frames
    y, uv = _nv12((4,), 96, 160, seed=11)
    mc, w = fixture(RID)
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.15, max_faces=M_FACES)
    bgr = N.nv12_to_bgr(y, uv)
    first = det.detect_images(bgr, crop='square')
    count = [len(r.scores) for r in first]
    print('faces per frame on the converted noise frames:', count)
    assert sum(count) >= 1                            # not vacuous
    return dict(det=det, fixture=(mc, w), y=y, uv=uv, bgr=bgr, nv12=NV12Frames(y, uv), first=first)


def _same(a, b, extra=()):
    for f in FIELDS + tuple(extra):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, f
        np.testing.assert_array_equal(x, y, err_msg=f)


def _same_lists(a, b, extra=()):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        _same(ra, rb, extra)


@pytest.mark.gpu
def test_gpu_detect_images_batch_and_faces(e2e):
    import torch
    from hpe.preprocess import NV12Frames
    det, f = e2e['det'], e2e['nv12']
    _same_lists(det.detect_images(f, crop='square'), e2e['first'])
    whole = det.detect_images(e2e['bgr'])
    _same_lists(det.detect_images(f), whole)
    _same_lists(det.detect_batch(f), whole)
    _same(det.detectFaces(f[2:3]), whole[2])
    on_device = NV12Frames(torch.from_numpy(e2e['y']).cuda(), torch.from_numpy(e2e['uv']).cuda())
    _same_lists(det.detect_images(on_device, crop='square'), e2e['first'])
    np.testing.assert_array_equal(det.prepare(f, crop='square').cpu().numpy(),
                                  det.prepare(e2e['bgr'], crop='square').cpu().numpy())
    with pytest.raises(ValueError, match='bgr'):
        det.detect_images(f, bgr=False)


@pytest.mark.gpu
def test_gpu_detect_rois_and_refine(e2e):
    det, f = e2e['det'], e2e['nv12']
    rois = np.array([(i % 4, x0, y0, s, s) for i, (x0, y0, s) in
                     enumerate([(10, 5, 80), (-20, -10, 90), (100, 30, 96), (33, 1, 64), (0, 0, 96), (70, 40, 100)])])
    a = det.detect_rois(f, rois, pad_value=PAD)
    b = det.detect_rois(e2e['bgr'], rois, pad_value=PAD)
    assert len(a) == len(rois)
    _same_lists(a, b)
    assert det.detect_rois(f, np.zeros((0, 5), np.int32)) == []
    for scale in (SCALE, 0.1):
        a = det.detect_refine(f, scale=scale, crop='square', pad_value=PAD)
        b = det.detect_refine(e2e['bgr'], scale=scale, crop='square', pad_value=PAD)
        _same_lists(a, b, extra=('refined',))
        print('detect_refine scale %g: %d of %d faces replaced' % (scale, sum(int(r.refined.sum()) for r in a),
                                                                   sum(len(r.scores) for r in a)))


@pytest.mark.gpu
def test_gpu_detect_tiled(e2e):
    det, f = e2e['det'], e2e['nv12']
    for kw in (dict(tile=64), dict(tile=48, overlap=8, crop='square', pad_value=PAD),
               dict(tile=64, roi_batch=7), dict(tile=200, full=False)):        # 7: chunks of whole frames
        a = det.detect_tiled(f, **kw)
        b = det.detect_tiled(e2e['bgr'], **kw)
        assert len(a) == 4
        _same_lists(a, b, extra=('roi', 'src'))
    assert det.detect_tiled(f[:0], 64) == []
    with pytest.raises(ValueError, match='bgr'):
        det.detect_tiled(f, 64, bgr=False)


@pytest.mark.gpu
def test_gpu_detect_video(e2e):
    from hpe.preprocess import NV12Frames
    from hpe.tracking import PoseTracker
    det = e2e['det']
    rep = 4
    yc, uvc = (np.repeat(p[:, None], rep, axis=1) for p in (e2e['y'], e2e['uv']))   # (4, 4, ...): 4 clips
    bc = np.repeat(e2e['bgr'][:, None], rep, axis=1)
    # one video, two calls in a row on one tracker
    for s in range(2):
        ta, tb = PoseTracker(device=det.device), PoseTracker(device=det.device)
        clip = NV12Frames(yc[s], uvc[s])
        a = det.detect_video(clip[:3], ta, crop='square') + det.detect_video(clip[3:], ta, crop='square')
        b = det.detect_video(bc[s][:3], tb, crop='square') + det.detect_video(bc[s][3:], tb, crop='square')
        assert len(a) == rep
        _same_lists(a, b, extra=('track',))
        for x, y in zip(ta.state(), tb.state()):
            np.testing.assert_array_equal(x, y)
    # four videos at once, two calls in a row
    ta, tb = PoseTracker(streams=4, device=det.device), PoseTracker(streams=4, device=det.device)
    for lo, hi in ((0, 1), (1, 4)):
        a = det.detect_video(NV12Frames(yc[:, lo:hi], uvc[:, lo:hi]), ta, crop='square')
        b = det.detect_video(bc[:, lo:hi], tb, crop='square')
        assert len(a) == 4
        for ra, rb in zip(a, b):
            _same_lists(ra, rb, extra=('track',))
    assert any((r.track >= 0).any() for ra in a for r in ra)
    for x, y in zip(ta.state(), tb.state()):
        np.testing.assert_array_equal(x, y)
    assert det.detect_video(NV12Frames(yc[0][:0], uvc[0][:0]), PoseTracker(device=det.device)) == []
    with pytest.raises(ValueError):
        det.detect_video(NV12Frames(yc[:3], uvc[:3]), ta, crop='square')          # 3 videos, 4 streams
    with pytest.raises(ValueError, match='bgr'):
        det.detect_video(NV12Frames(yc[0], uvc[0]), PoseTracker(device=det.device), bgr=False)


@pytest.mark.gpu
def test_gpu_feature_extractor(e2e, tmp_path):
    from hpe.features import FeatureExtractor
    mc, w = e2e['fixture']
    f = e2e['nv12']
    fe = FeatureExtractor(mc, w, scoreThreshold=0.15, max_faces=M_FACES)
    a = {k: v.cpu().numpy() for k, v in fe.extract_device(f, crop='square').items()}
    b = {k: v.cpu().numpy() for k, v in fe.extract_device(e2e['bgr'], crop='square').items()}
    assert set(a) == set(b)
    for k in ('count', 'src', 'feat88', 'feat96'):
        np.testing.assert_array_equal(a[k], b[k])
    for i in range(4):
        c = int(a['count'][i])
        for k in ('det_index', 'scores', 'boxes', 'keypoints', 'poses'):
            np.testing.assert_array_equal(a[k][i, :c], b[k][i, :c])
    assert a['count'].sum() >= 1
    # host arrays in slices of frames, and of ROI rows
    rois = np.array([(i % 4, x0, y0, s, s) for i, (x0, y0, s) in
                     enumerate([(10, 5, 80), (-20, -10, 90), (100, 30, 96), (33, 1, 64), (0, 0, 96)])])
    for kw in (dict(crop='square'), dict(rois=rois, pad_value=PAD)):
        ea = fe.extract(f, batch_size=3, **kw)
        eb = fe.extract(e2e['bgr'], batch_size=3, **kw)
        for x, y in zip(ea, eb):
            assert x.dtype == y.dtype
            np.testing.assert_array_equal(x, y)
    poses = np.arange(12.0).reshape(4, 3)
    pa = fe.build_datasets(f, poses, str(tmp_path / 'nv12'), batch_size=3, crop='square')
    pb = fe.build_datasets(e2e['bgr'], poses, str(tmp_path / 'bgr'), batch_size=3, crop='square')
    for x, y in zip(pa, pb):
        dx, dy = np.load(x), np.load(y)
        np.testing.assert_array_equal(dx['features'], dy['features'])
        np.testing.assert_array_equal(dx['poses'], dy['poses'])
    with pytest.raises(ValueError, match='bgr'):
        fe.extract_device(f, bgr=False)
