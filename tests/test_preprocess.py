"""Raw uint8 frames -> network input (hpe.preprocess, csrc/hpe_preproc.hip, C ABI hpe_preprocess).

CPU: the fp32 restatement of TF's ResizeBicubic (tests/bicubic_ref.py) is pinned to Pillow where the
two algorithms agree (float images, upscales: Pillow's BICUBIC is Keys A = -0.5 with clipped-window
renormalisation and no antialiasing), to exact cases, and to its own float64 evaluation; the C entry
point's argument checks and the Python surface are exercised without a device.
GPU: the kernel equals the restatement bit for bit on every path (identity, up / down scale, fewer
than four source pixels, crop + row stride, channel order, the detector's real geometry, offsets past
2^32 bytes), and the uint8 entry points of the detector and the feature extractor equal their float
entry points fed the restatement's floats.

TF parity itself is unpinned (TensorFlow is absent, as for the rest of the oracle): the restatement is
TF's arithmetic written out, not TF output."""
import ctypes
import os

import numpy as np
import pytest

import bicubic_ref as B
from hpe import _lib
from util import fixture

RID = 'reg1-stoqa9pt-reg2-hrchr82r-selected'
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the restatement ---------------------------------------------------------------------------

def _pillow(a, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.Resampling.BICUBIC))


@pytest.mark.parametrize('h,w,oh,ow,tol', [(8, 8, 16, 16, 1e-6), (5, 7, 20, 28, 1e-6), (6, 9, 13, 11, 2e-3)])
def test_restatement_matches_pillow_on_upscales(h, w, oh, ow, tol):
    """Integer upscales hit table entries exactly (1e-6); 6x9 -> 13x11 sees the 1/1024 quantisation
    of the table offset (2e-3).  Downscales are not compared: Pillow antialiases, TF does not."""
    a = np.random.default_rng(h * 100 + w).random((h, w)).astype(np.float32)
    got = B.resize(a[None, :, :, None], oh, ow)[0, :, :, 0]
    err = np.abs(got - _pillow(a, oh, ow)).max()
    print('pillow %dx%d -> %dx%d: max |diff| %.3g' % (h, w, oh, ow, err))
    assert err <= tol


def test_same_size_resize_is_exact():
    a = np.random.default_rng(0).random((2, 9, 7, 3)).astype(np.float32)
    np.testing.assert_array_equal(B.resize(a, 9, 7), a)


@pytest.mark.parametrize('h,w,oh,ow', [(8, 8, 16, 16), (6, 9, 13, 11), (23, 17, 8, 8), (2, 3, 8, 8)])
def test_constant_image_stays_constant(h, w, oh, ow):
    """Within 1 ulp, taken at the top of the value range: 2^-24, the spacing of fp32 below 1."""
    a = np.full((1, h, w, 1), 0.3, np.float32)
    err = np.abs(B.resize(a, oh, ow) - np.float32(0.3)).max()
    print('constant %dx%d -> %dx%d: max |diff| %.3g' % (h, w, oh, ow, err))
    assert err <= 2.0 ** -24


def test_weight_table_and_borders():
    near, far = B.coeffs()
    assert near[0] == 1 and near[1024] == 0 and far[0] == 0 and far[1024] == 0
    idx, w = B.weights(8, 8)                         # identity: the tap itself, weight 1
    np.testing.assert_array_equal(idx[:, 1], np.arange(8))
    np.testing.assert_array_equal(w, np.tile(np.float32([0, 1, 0, 0]), (8, 1)))
    idx, w = B.weights(4, 1)                         # one source pixel: every tap clamps to it
    assert (idx == 0).all()
    np.testing.assert_allclose(w.sum(1), 1, atol=2e-7)
    assert ((w != 0).sum(1) == 1).all()


@pytest.mark.parametrize('h,w,size,crop', [(23, 17, 8, None), (5, 7, (20, 28), None), (2, 3, 8, None),
                                           (96, 160, 128, 'square'), (13, 19, 8, (3, 2, 9, 8))])
def test_fp32_restatement_against_float64(h, w, size, crop):
    """12 roundings x 2^-24 x sum |wy||wx| (<= 1.5625) x 2 for the final scaling = 2.3e-6, doubled."""
    u8 = _u8((2, h, w, 3), seed=h + w)
    got, ref = B.preprocess(u8, size, crop=crop), B.preprocess_f64(u8, size, crop=crop)
    assert got.dtype == np.float32 and ref.dtype == np.float64 and got.shape == ref.shape
    print('fp32 vs fp64 %dx%d: max |diff| %.3g' % (h, w, np.abs(got - ref).max()))
    np.testing.assert_allclose(got, ref, rtol=0, atol=5e-6)


def test_tap_values_and_channel_order():
    u8 = _u8((1, 4, 5, 3), seed=3)
    v = B.tap_values(u8, bgr=True)
    np.testing.assert_array_equal(v, (u8[..., ::-1] / 255.0).astype(np.float32))
    np.testing.assert_array_equal(B.tap_values(u8[..., ::-1], bgr=False), v)
    assert B.crop_rect(480, 640, 'square') == (80, 0, 480, 480)
    assert B.crop_rect(7, 4, 'square') == (0, 1, 4, 4)


# ---- interface, no device ----------------------------------------------------------------------

def test_signature_is_bound():
    assert 'hpe_preprocess' in _lib.SIGNATURES


@built
def test_hpe_preprocess_rejects_bad_arguments():
    lib = _lib.load()
    z = ctypes.c_void_p(256)

    def call(frames=z, n=1, in_h=8, in_w=8, stride=24, crop=(0, 0, 8, 8), out=z, out_h=4, out_w=4):
        return lib.hpe_preprocess(frames, n, in_h, in_w, stride, crop[0], crop[1], crop[2], crop[3], 1, out,
                                  out_h, out_w, None)

    assert call(frames=None) == 1
    assert b'hpe_preprocess' in lib.hpe_last_error() and b'null' in lib.hpe_last_error()
    assert call(out=None) == 1
    assert call(crop=(4, 0, 8, 8)) == 1             # past the right edge
    assert b'crop' in lib.hpe_last_error()
    assert call(crop=(0, 1, 8, 8)) == 1             # past the bottom edge
    assert call(crop=(-1, 0, 4, 4)) == 1
    assert call(stride=23) == 1
    assert b'stride' in lib.hpe_last_error()
    assert call(out_w=0) == 1
    assert call(in_h=0) == 1
    assert call(n=1 << 40, out_h=128, out_w=128) == 1   # n * out_h * out_w above INT32_MAX
    assert b'INT32_MAX' in lib.hpe_last_error()
    assert call(n=0) == 0
    assert call(frames=None, out=None, n=0) == 0


def test_ema_filter():
    from hpe.detector import EMAFilter
    f = EMAFilter(0.25)
    assert f.update(8.0) == 8.0                      # the first measurement passes through
    assert f.update(4.0) == 0.25 * 4.0 + 0.75 * 8.0
    s = f.state
    assert f.update(-2.0) == 0.25 * -2.0 + (1.0 - 0.25) * s
    with pytest.raises(AssertionError):
        EMAFilter(0.0)


def test_prepare_input_rejects_non_uint8_and_wrong_rank():
    import torch
    from hpe.preprocess import prepare_input
    with pytest.raises(ValueError):
        prepare_input(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        prepare_input(torch.zeros((1, 8, 8, 3)))
    with pytest.raises(ValueError):
        prepare_input(np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError):
        prepare_input(np.zeros((1, 1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        prepare_input(np.zeros((8, 8, 4), np.uint8))


# ---- the kernel --------------------------------------------------------------------------------

def _gpu(frames, **kw):
    from hpe.preprocess import prepare_input
    return prepare_input(frames, **kw).cpu().numpy()


# (n, H, W), size, crop
CASES = {
    'identity': ((2, 8, 8), 8, None),
    'upscale_nonsquare': ((1, 5, 7), (20, 28), None),
    'downscale_noninteger': ((1, 23, 17), 8, None),
    'one_pixel': ((1, 1, 1), 4, None),
    'two_by_three': ((1, 2, 3), 8, None),
    'odd_output': ((1, 6, 9), (13, 11), None),
    'webcam_front': ((3, 480, 640), 128, 'square'),
    'back_model': ((1, 300, 300), 256, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_gpu_kernel_equals_restatement(name):
    shape, size, crop = CASES[name]
    u8 = _u8(shape + (3,), seed=len(name))
    want = B.preprocess(u8, size, crop=crop)
    got = _gpu(u8, size=size, crop=crop)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_gpu_crop_and_row_stride():
    """A 13 x 19 frame cut out of a wider device tensor (row stride > 3 * in_w), read in place."""
    import torch
    wide = _u8((2, 13, 31, 3), seed=5)
    dev = torch.from_numpy(wide).cuda()
    view = dev[:, :, 4:23]
    assert not view.is_contiguous() and view.stride(1) == 31 * 3
    want = B.preprocess(wide[:, :, 4:23], 8, crop=(3, 2, 9, 8))
    np.testing.assert_array_equal(_gpu(view, size=8, crop=(3, 2, 9, 8)), want)
    # the host array and a single (H, W, 3) frame take the same kernel
    np.testing.assert_array_equal(_gpu(wide[:, :, 4:23], size=8, crop=(3, 2, 9, 8)), want)
    np.testing.assert_array_equal(_gpu(wide[1, :, 4:23], size=8, crop=(3, 2, 9, 8)), want[1:])
    with pytest.raises(ValueError):
        _gpu(view, size=8, crop=(12, 2, 9, 8))


@pytest.mark.gpu
def test_gpu_channel_order():
    u8 = _u8((2, 11, 14, 3), seed=9)
    a = _gpu(u8, size=(9, 16), bgr=True)
    np.testing.assert_array_equal(_gpu(np.ascontiguousarray(u8[..., ::-1]), size=(9, 16), bgr=False), a)
    np.testing.assert_array_equal(a, B.preprocess(u8, (9, 16), bgr=True))
    np.testing.assert_array_equal(_gpu(u8, size=(9, 16), bgr=False), B.preprocess(u8, (9, 16), bgr=False))


@pytest.mark.gpu
def test_gpu_offsets_past_4_gib():
    """342 frames of 2048 x 2048 x 3 bytes (4.3 GB): frame 341 starts past 2^31 and its lower tap
    rows lie past 2^32 bytes.  The ROI kernel's frame and row address sums feed the same loads: two
    full-frame rows give what the crop kernel gives."""
    import torch
    from hpe.preprocess import prepare_input, prepare_rois
    n, s = 342, 2048
    if torch.cuda.mem_get_info()[0] < 6 * 1024 ** 3:
        pytest.skip('needs 6 GB of free device memory')
    assert (n - 1) * s * s * 3 > 2 ** 31 and ((n - 1) * s + s * 3 // 4) * s * 3 > 2 ** 32
    g = torch.Generator(device='cuda').manual_seed(7)
    dev = torch.randint(0, 256, (n, s, s, 3), dtype=torch.uint8, device='cuda', generator=g)
    got = prepare_input(dev, size=8)[[0, n - 1]].cpu().numpy()
    rois = prepare_rois(dev, [(0, 0, 0, s, s), (n - 1, 0, 0, s, s)], size=8).cpu().numpy()
    ends = dev[[0, n - 1]].cpu().numpy()
    del dev
    np.testing.assert_array_equal(got, B.preprocess(ends, 8))
    np.testing.assert_array_equal(rois, got)


# ---- end to end: the uint8 entry points equal the float entry points -----------------------------

@pytest.fixture(scope='module')
def e2e():
    u8 = _u8((4, 96, 160, 3), seed=11)
    return u8, B.preprocess(u8, 128, crop='square')


@pytest.mark.gpu
def test_gpu_forward_of_prepared_frames(e2e):
    import torch
    from hpe.blazeface import BlazeFace
    from hpe.preprocess import prepare_input
    u8, ref = e2e
    net = BlazeFace(*fixture(RID))
    a = [o.cpu().numpy() for o in net.forward(prepare_input(u8, crop='square'))]
    b = [o.cpu().numpy() for o in net.forward(torch.from_numpy(ref).cuda())]
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_detect_images_equals_detect_batch(e2e):
    from hpe.detector import BlazeFaceDetector
    u8, ref = e2e
    mc, w = fixture(RID)
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.15, max_faces=8)
    a = det.detect_images(u8, crop='square')
    b = det.detect_batch(ref)
    assert len(a) == len(b) == 4
    for ra, rb in zip(a, b):
        for f in ('boxes', 'keypoints', 'scores', 'poses'):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f))
    # uint8 dispatch of the reference's call shape: detectFaces(frame) on a raw BGR frame
    sq = np.ascontiguousarray(u8[:, :, 32:128])
    c = det.detect_batch(sq)
    d = det.detectFaces(sq[2])
    for f in ('boxes', 'keypoints', 'scores', 'poses'):
        np.testing.assert_array_equal(getattr(d, f), getattr(b[2], f))
        for rc, rb in zip(c, b):
            np.testing.assert_array_equal(getattr(rc, f), getattr(rb, f))


@pytest.mark.gpu
def test_gpu_feature_extractor_takes_uint8(e2e):
    from hpe.features import FeatureExtractor
    u8, ref = e2e
    mc, w = fixture(RID)
    fe = FeatureExtractor(mc, w, scoreThreshold=0.15, max_faces=8)
    a = {k: v.cpu().numpy() for k, v in fe.extract_device(u8, crop='square').items()}
    b = {k: v.cpu().numpy() for k, v in fe.extract_device(ref).items()}
    assert set(a) == set(b) and {'feat88', 'feat96', 'src', 'count'} <= set(a)
    for k in ('count', 'src', 'feat88', 'feat96'):
        np.testing.assert_array_equal(a[k], b[k])
    for i in range(4):
        c = int(a['count'][i])
        for k in ('det_index', 'scores', 'boxes', 'keypoints', 'poses'):
            np.testing.assert_array_equal(a[k][i, :c], b[k][i, :c])
    ea = fe.extract(u8, batch_size=3, crop='square')
    eb = fe.extract(ref, batch_size=3)
    for x, y in zip(ea, eb):
        np.testing.assert_array_equal(x, y)
