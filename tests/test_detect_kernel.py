"""hpe_detect and hpe_gather_features (csrc/hpe_detect.hip) called through ctypes on plain numpy
inputs, the outputs pre-filled with sentinels, against oracle.detector_ref.

Reference: tests/detect_ref.py restates the oracle's detect_frame with a vectorised float32 NMS; the
CPU tests hold the two equal, state the condition under which the kept order cannot depend on whose
exp computed the scores, and check the seeded search for box pairs whose IoU moves when the
denominator is contracted into a fused multiply-add.

Bars (GPU): count, det_index and poses equal; float64 boxes and keypoints bit for bit (the decode
multiplies by powers of two only); slots past count still the sentinel; scores
|got - s| <= 2^-22 * s with s the float64 sigmoid of the logit: one ulp for expf (HIP's documented
bound, 2^-23 relative) plus one rounding each for the add and the divide (2 * 2^-24).  Where s is below
the float32 range (logits <= -100 here, see tests/detect_ref.py) the score must be exactly 0.0f.
The largest measured ratio to the bound is printed and recorded in DESIGN.md.
hpe_gather_features equals oracle.detector_ref.gather_features bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import detect_ref as R
from hpe import _lib
from oracle import detector_ref as D

built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')
F4, F8 = np.float32, np.float64
SENTINEL = dict(count=-7, det_index=-9, scores=77.0, boxes=1e300, keypoints=1e300, poses=77.0)
OUT_KEYS = ('det_index', 'scores', 'boxes', 'keypoints', 'poses')


@pytest.fixture(scope='module')
def cases():
    return R.cases()


@pytest.fixture(scope='module')
def pairs():
    return R.iou_pairs()


_reference = {}


def reference(name, c):
    """The restatement's per-frame results of a named case, computed once."""
    if name not in _reference:
        _reference[name] = [R.detect_frame(fr, c['t'], c['iou'], c['max_faces']) for fr in c['frames']]
    return _reference[name]


def _same_result(a, b, what):
    np.testing.assert_array_equal(a['det_index'], b['det_index'], err_msg=what)
    for k in ('scores', 'boxes', 'keypoints', 'poses'):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- CPU: the restatement, the order condition, the pair search, the host checks --------------------

def test_restatement_equals_oracle(cases):
    seen = 0
    for name, c in cases.items():
        for f, fr in enumerate(c['frames']):
            if len(R.candidates(fr, c['t'])) > 64:
                continue
            want = R.oracle_frame(fr, c['t'], c['iou'], c['max_faces'])
            _same_result(reference(name, c)[f], want, '%s frame %d' % (name, f))
            seen += 1
    assert seen >= 12
    for seed, k in ((60, 90), (61, 150), (62, 200)):
        fr = R.random_frame(seed, k)
        _same_result(R.detect_frame(fr), R.oracle_frame(fr), 'random frame %d' % seed)
    for fr, _, _ in R.exact_third_frames():
        for thr in (F4(1 / 3), np.nextafter(F4(1 / 3), F4(0))):
            _same_result(R.detect_frame(fr, iou_threshold=thr), R.oracle_frame(fr, iou_threshold=thr), 'third')


def test_restatement_iou_equals_oracle_iou():
    rng = np.random.default_rng(63)
    b = rng.uniform(0, 1, (300, 2, 4)).astype(F4)       # corners in any order
    b[::7, 0, 2] = b[::7, 0, 0]                         # some of zero area
    got = R.iou(b[:, 0], b[:, 1])
    for i in range(len(b)):
        assert got[i].tobytes() == D._iou(b[i, 0], b[i, 1]).tobytes()
    assert (got > 0).sum() > 100 and (got == 0).sum() > 40
    # The areas that are not positive, on either side (tests/track_ref.py leans on this too): zero
    # (no width, no height, a point) and NaN (inf - inf from float64 values beyond the float32 range,
    # inf * 0 from a height that overflows on a box of no width).  The kernels' rule is IoU 0; the oracle
    # gives 0 for the zero areas and lets a NaN area through as a NaN IoU, which suppresses and matches
    # nothing either.
    big = F4(3e38)
    good = F4([0.1, 0.2, 0.5, 0.7])
    odd = {'no width': F4([0.1, 0.3, 0.5, 0.3]), 'no height': F4([0.4, 0.2, 0.4, 0.7]),
           'a point': F4([0.3, 0.3, 0.3, 0.3]), 'inf - inf': F4([np.inf, 0.2, np.inf, 0.7]),
           'inf * 0': F4([-big, 0.3, big, 0.3]), '-inf - -inf': F4([0.1, -np.inf, 0.5, -np.inf])}
    for name, o in odd.items():
        for bi, bj in ((o, good), (good, o), (o, o), (o[[2, 3, 0, 1]], good)):
            v = R.iou(bi, bj)
            assert v.dtype == F4 and v.tobytes() == F4(0).tobytes(), name
            with np.errstate(all='ignore'):
                w = D._iou(bi, bj)
            assert w.tobytes() == F4(0).tobytes() if 'inf' not in name else np.isnan(w), name


def test_cases_expected_shape(cases):
    """What each case is there for does happen in its reference result."""
    n = lambda name, f=0: len(reference(name, cases[name])[f]['det_index'])   # noqa: E731
    for t in (0.4, 0.5, 1e-30):
        c = cases['threshold_%g' % t]
        fr, ref = c['frames'][0], reference('threshold_%g' % t, c)[0]
        thr = R.logit_threshold(t)
        up = np.nextafter(thr, F4(np.inf))
        kept = np.where((fr['cls'] == up) | (fr['cls'] == np.inf))[0]
        assert sorted(ref['det_index']) == kept.tolist() and (fr['cls'] == up).sum() == 7
        assert (ref['scores'][np.isinf(fr['cls'][ref['det_index']])] == 1).all()
        assert (fr['cls'] == thr).sum() >= 7 and np.isnan(fr['cls']).sum() == 7
    assert (cases['threshold_0.5']['frames'][0]['cls'] == 0).sum() == 21          # the threshold, +0 and -0
    assert R.logit_threshold(0.5) == 0 and R.logit_threshold(0.0) == -np.inf
    ref = reference('threshold_minus_inf_mixed', cases['threshold_minus_inf_mixed'])[0]
    cls = cases['threshold_minus_inf_mixed']['frames'][0]['cls']
    assert sorted(ref['det_index']) == np.where(np.isfinite(cls) | (cls == np.inf))[0].tolist()
    ref = reference('saturated_high', cases['saturated_high'])[0]
    assert (ref['scores'] == 1).all() and (np.diff(ref['det_index']) > 0).all() and 5 < len(ref['scores']) < 50
    for name, k in (('saturated_low_896', 896), ('saturated_low_40', 40)):
        ref = reference(name, cases[name])[0]
        assert len(R.candidates(cases[name]['frames'][0], 0.0)) == k
        assert (ref['scores'] == 0).all() and (np.diff(ref['det_index']) > 0).all() and 5 < len(ref['scores']) < k
    for m in (1, 7, 100, 896, 1000):
        assert n('all_anchors_max_%d' % m) == min(m, 896)
    assert sorted(reference('all_anchors_max_896', cases['all_anchors_max_896'])[0]['det_index']) == list(range(896))
    fr = cases['flipped']['frames'][0]
    on = R.candidates(fr, 0.4)
    assert (fr['loc'][on, 2] < 0).sum() > 10 and (fr['loc'][on, 3] < 0).sum() > 10 and 3 < n('flipped') < 48
    assert sorted(reference('zero_area', cases['zero_area'])[0]['det_index']) == [3, 10, 11, 12, 20, 21, 30, 700, 701]
    assert reference('contained', cases['contained'])[0]['det_index'].tolist() == [0, 300, 520, 301]
    fr = cases['same_box_896']['frames'][0]
    assert len(R.candidates(fr, 0.4)) == 896
    assert reference('same_box_896', cases['same_box_896'])[0]['det_index'].tolist() == [int(np.argmax(fr['cls']))]
    assert [len(R.candidates(fr, 0.4)) for fr in cases['counts']['frames']] == list(R.COUNTS)
    assert n('counts', 5) == 120 and 20 < n('counts', 4) < 120 and n('counts', 0) == 0 and n('counts', 1) == 1


def test_order_does_not_depend_on_exp(cases, pairs):
    for name, c in cases.items():
        for f, fr in enumerate(c['frames']):
            assert R.order_safe(fr, c['t']), (name, f)
    for a, b, _ in pairs[0] + pairs[1]:
        assert R.order_safe(R.pair_frame(a, b), 0.4)
    for fr, _, _ in R.exact_third_frames():
        assert R.order_safe(fr, 0.4)
    assert R.order_safe(R.nonfinite_frame(), 0.4)
    # the condition does refuse what it is there to refuse
    fr = R.blank(0)
    fr['cls'][:2] = [F4(3.0), np.nextafter(F4(3.0), F4(4))]
    assert not R.order_safe(fr, 0.4)
    fr['cls'][:2] = [F4(3.0), F4(-90.0)]
    assert R.order_safe(fr, 0.4) and not R.order_safe(fr, 0.0)
    fr['cls'][:2] = [F4(25.0), F4(12.0)]
    assert not R.order_safe(fr, 0.4)


def test_iou_pair_search_yields(pairs):
    higher, lower = pairs
    assert len(higher) >= 8 and len(lower) >= 8
    for group, sign in ((higher, 1), (lower, -1)):
        for a, b, ref in group:
            fr = R.pair_frame(a, b)
            boxes, _ = R.decode(fr['loc'], np.arange(2))
            b32 = boxes.astype(F4)
            assert R.iou(b32[0], b32[1]).tobytes() == ref.tobytes() == D._iou(b32[0], b32[1]).tobytes()
            con = R.iou_contracted(b32[0], b32[1])
            assert (con > ref) if sign > 0 else (con < ref), (con, ref)
            assert abs(float(con) - float(ref)) <= 2 * np.spacing(ref)          # an ulp or two
            # at the reference IoU both are kept, one float32 below it the second is suppressed
            assert R.oracle_frame(fr, iou_threshold=ref)['det_index'].tolist() == [0, 1]
            assert R.oracle_frame(fr, iou_threshold=np.nextafter(ref, F4(0)))['det_index'].tolist() == [0]


def _detect_args(**over):
    z = ctypes.c_void_p(256)
    a = dict(cls0=z, cls1=z, loc0=z, loc1=z, pose0=z, pose1=z, n=1, thr=0.0, iou=0.3, max_faces=4, count=z,
             det_index=z, scores=z, boxes=z, keypoints=z, poses=z)
    a.update(over)
    return [a[k] for k in ('cls0', 'cls1', 'loc0', 'loc1', 'pose0', 'pose1', 'n', 'thr', 'iou', 'max_faces', 'count',
                           'det_index', 'scores', 'boxes', 'keypoints', 'poses')] + [None]


@built
def test_hpe_detect_rejects_bad_arguments():
    lib = _lib.load()
    for k in ('cls0', 'cls1', 'loc0', 'loc1', 'pose0', 'pose1', 'count', 'det_index', 'scores', 'boxes', 'keypoints',
              'poses'):
        assert lib.hpe_detect(*_detect_args(**{k: None})) == 1, k
        assert b'hpe_detect' in lib.hpe_last_error() and b'null' in lib.hpe_last_error()
    for m in (0, -1, -2 ** 31):
        assert lib.hpe_detect(*_detect_args(max_faces=m)) == 1, m
        assert b'max_faces' in lib.hpe_last_error()
    for n in (2 ** 31, 2 ** 40):
        assert lib.hpe_detect(*_detect_args(n=n)) == 1, n
        assert b'too large' in lib.hpe_last_error()
    assert lib.hpe_detect(*_detect_args(n=0)) == 0
    assert lib.hpe_detect(*_detect_args(n=0, max_faces=0)) == 1


# ---- GPU: hpe_detect ---------------------------------------------------------------------------------

def gpu_detect(frames, thr, iou, max_faces):
    """hpe_detect on a batch of frame dicts; thr is the float32 logit threshold as the C ABI takes it."""
    import torch
    lib = _lib.load()
    n, M = len(frames), int(max_faces)
    host = [np.stack([fr['cls'][:R.N0] for fr in frames]), np.stack([fr['cls'][R.N0:] for fr in frames]),
            np.stack([fr['loc'][:R.N0] for fr in frames]), np.stack([fr['loc'][R.N0:] for fr in frames]),
            np.stack([fr['pose0'] for fr in frames]), np.stack([fr['pose1'] for fr in frames])]
    assert all(h.dtype == F4 for h in host)
    assert [h.shape[1:] for h in host] == [(512,), (384,), (512, 16), (384, 16), (16, 16, 3), (8, 8, 3)]
    dev = [torch.from_numpy(np.ascontiguousarray(h)).cuda() for h in host]
    full = lambda shape, k, dt: torch.full(shape, SENTINEL[k], dtype=dt, device='cuda')   # noqa: E731
    out = dict(count=full((n,), 'count', torch.int32), det_index=full((n, M), 'det_index', torch.int32),
               scores=full((n, M), 'scores', torch.float32), boxes=full((n, M, 4), 'boxes', torch.float64),
               keypoints=full((n, M, 6, 2), 'keypoints', torch.float64), poses=full((n, M, 3), 'poses', torch.float32))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(lib.hpe_detect(*[p(d) for d in dev], n, float(F4(thr)), float(F4(iou)), M, p(out['count']),
                              p(out['det_index']), p(out['scores']), p(out['boxes']), p(out['keypoints']),
                              p(out['poses']), None), 'hpe_detect')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _unwritten(got, f, c):
    for k in OUT_KEYS:
        assert (got[k][f, c:] == SENTINEL[k]).all(), 'frame %d: slots past the count were written: %s' % (f, k)


def _check_frame(got, f, fr, want):
    """Frame f of the kernel's outputs against the restatement's result `want`; returns the largest
    score error over the bound."""
    c = int(got['count'][f])
    assert c == len(want['det_index']), (f, c, len(want['det_index']))
    np.testing.assert_array_equal(got['det_index'][f, :c], want['det_index'])
    assert got['poses'][f, :c].tobytes() == want['poses'].tobytes()
    assert got['boxes'][f, :c].tobytes() == want['boxes'].tobytes()
    assert got['keypoints'][f, :c].tobytes() == want['keypoints'].tobytes()
    _unwritten(got, f, c)
    s = R.sigmoid64(fr['cls'][want['det_index']])
    sc = got['scores'][f, :c]
    inside = s >= np.finfo(F4).tiny
    assert (sc[~inside] == 0).all() and not np.signbit(sc).any()
    ratio = np.abs(sc.astype(F8) - s)[inside] / (R.SCORE_BOUND * s[inside])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, 'score error %.3f of the 2^-22 bound' % worst
    return worst


def _run_case(name, c):
    got = gpu_detect(c['frames'], R.logit_threshold(c['t']), c['iou'], c['max_faces'])
    worst = max([_check_frame(got, f, fr, w) for f, (fr, w) in enumerate(zip(c['frames'], reference(name, c)))])
    print('%s: largest score error / bound %.3f' % (name, worst))
    return got


CASE_NAMES = ['threshold_0.4', 'threshold_0.5', 'threshold_1e-30', 'threshold_minus_inf', 'threshold_minus_inf_mixed',
              'saturated_high', 'saturated_low_896', 'saturated_low_40', 'all_anchors_max_1', 'all_anchors_max_7',
              'all_anchors_max_100', 'all_anchors_max_896', 'all_anchors_max_1000', 'flipped', 'zero_area', 'contained',
              'same_box_896', 'disjoint', 'six_frames']


def test_case_names_are_all_cases(cases):
    assert sorted(CASE_NAMES + ['counts']) == sorted(cases)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_gpu_detect_case(cases, name):
    got = _run_case(name, cases[name])
    if name.startswith('saturated_high'):
        assert (got['scores'][0, :got['count'][0]] == 1).all()
    if name.startswith('saturated_low'):
        assert (got['scores'][0, :got['count'][0]] == 0).all()


@pytest.mark.gpu
def test_gpu_detect_score_error_sweep():
    """Every multiple of 1/64 in [-8, 8] and a spread of logits down to the threshold of t = 1e-30, all
    kept (disjoint boxes): the score bound over the whole range the other cases draw from."""
    fr = R.all_anchors_frame(70)
    fr['cls'][:] = (np.arange(896) / 64.0 - 6.0).astype(F4)
    lo = R.all_anchors_frame(71)
    lo['cls'][:] = (-np.arange(896) * (63.0 / 896) - 6.0).astype(F4)
    c = R.case([fr, lo], t=1e-30, max_faces=896)
    assert lo['cls'].min() > R.logit_threshold(1e-30) and fr['cls'].max() <= 8
    got = gpu_detect(c['frames'], R.logit_threshold(c['t']), c['iou'], 896)
    assert got['count'].tolist() == [896, 896]
    worst = 0.0
    for f, x in enumerate((fr, lo)):
        s = R.sigmoid64(x['cls'][got['det_index'][f]])
        worst = max(worst, float((np.abs(got['scores'][f].astype(F8) - s) / (R.SCORE_BOUND * s)).max()))
    print('score sweep: largest score error / bound %.3f' % worst)
    assert worst <= 1.0


def _pair_launch(fr, thr):
    got = gpu_detect([fr], R.logit_threshold(0.4), thr, 100)
    c = int(got['count'][0])
    _unwritten(got, 0, c)
    return got['det_index'][0, :c].tolist()


@pytest.mark.gpu
def test_gpu_detect_iou_at_the_threshold(pairs):
    """Pairs whose IoU a contracted denominator moves by one float32: with the threshold on the pair's
    own IoU both are kept, one float32 below it the lower-scored one is suppressed.  (A kernel that
    fuses the multiply into the subtraction fails the first for the `higher` pairs and the second for
    the `lower` ones.)"""
    higher, lower = pairs
    failed = []
    for kind, group in (('higher', higher), ('lower', lower)):
        for i, (a, b, ref) in enumerate(group):
            fr = R.pair_frame(a, b)
            at, below = _pair_launch(fr, ref), _pair_launch(fr, np.nextafter(ref, F4(0)))
            if at != [0, 1] or below != [0]:
                failed.append((kind, i, float(ref), at, below))
    print('IoU at the threshold: %d of %d pairs fail' % (len(failed), len(higher) + len(lower)))
    assert not failed, failed


@pytest.mark.gpu
def test_gpu_detect_iou_exact_third():
    third = F4(1 / 3)
    for fr, d0, d1 in R.exact_third_frames():
        assert _pair_launch(fr, third) == [d0, d1]
        assert _pair_launch(fr, np.nextafter(third, F4(0))) == [d0]
        assert _pair_launch(fr, 0.3) == [d0]


@pytest.mark.gpu
def test_gpu_detect_candidate_counts(cases):
    """0, 1, 255, 256, 257 and 896 candidates in one batch (the workgroup has 256 threads): each frame
    equals the restatement, and the same frame launched alone bit for bit."""
    c = cases['counts']
    got = _run_case('counts', c)
    for f, fr in enumerate(c['frames']):
        alone = gpu_detect([fr], R.logit_threshold(c['t']), c['iou'], c['max_faces'])
        for k in ('count',) + OUT_KEYS:
            assert alone[k][0].tobytes() == got[k][f].tobytes(), (f, k)


@pytest.mark.gpu
def test_gpu_detect_batch_above_cu_count(cases):
    """300 frames (an MI355X has 256 CUs) cycling through six: the first six equal the restatement,
    every later copy its first occurrence bit for bit."""
    c = cases['six_frames']
    got = gpu_detect([c['frames'][i % 6] for i in range(300)], R.logit_threshold(c['t']), c['iou'], c['max_faces'])
    for f, (fr, w) in enumerate(zip(c['frames'], reference('six_frames', c))):
        _check_frame(got, f, fr, w)
    for k in ('count',) + OUT_KEYS:
        a = got[k].reshape(50, 6, -1)
        assert (a.view(np.uint8) == a[:1].view(np.uint8)).all(), k


@pytest.mark.gpu
def test_gpu_detect_nonfinite_loc_stays_in_its_frame(cases):
    """NaN / inf box values are outside the equality claims (the kernel's header says what happens);
    the frame's neighbours are unaffected and its count stays in range."""
    c = cases['six_frames']
    a, b, bad = c['frames'][0], c['frames'][3], R.nonfinite_frame()
    thr = R.logit_threshold(0.4)
    got = gpu_detect([a, bad, b, bad], thr, 0.3, 100)
    clean = gpu_detect([a, b], thr, 0.3, 100)
    for k in ('count',) + OUT_KEYS:
        assert got[k][0].tobytes() == clean[k][0].tobytes() and got[k][2].tobytes() == clean[k][1].tobytes(), k
    ref = reference('six_frames', c)
    _check_frame(got, 0, a, ref[0])
    _check_frame(got, 2, b, ref[3])
    for f in (1, 3):
        n = int(got['count'][f])
        assert 0 <= n <= 100
        _unwritten(got, f, n)
        on = set(R.candidates(bad, 0.4).tolist())
        assert set(got['det_index'][f, :n].tolist()) <= on and len(set(got['det_index'][f, :n].tolist())) == n
    for k in ('count',) + OUT_KEYS:
        a1, a3 = got[k][1], got[k][3]
        nan = np.isnan(a1) if a1.dtype.kind == 'f' else np.zeros(a1.shape, bool)
        assert (a1[~nan].tobytes() == a3[~nan].tobytes()), k


def gpu_merge_identity(scores, boxes, kps, iou, K, rows, M):
    """hpe_merge_rois on one frame of `rows` table rows, each the 1 x 1 ROI, with a 1 x 1 destination: the
    remap is ((0 + x * 1) - 0) / 1, the identity in bits.  The candidates (float32 scores, float64 boxes
    and keypoints) fill the rows' M slots in order.  Returns (src_out, boxes_out) of the kept ones."""
    import torch
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    n = len(scores)
    assert n <= rows * M
    count = np.asarray([min(max(n - r * M, 0), M) for r in range(rows)], np.int32)
    pad = lambda a: np.concatenate([a, np.zeros((rows * M - n,) + a.shape[1:], a.dtype)])   # noqa: E731
    rois = np.tile(np.asarray([0, 0, 0, 1, 1], np.int32), (rows, 1))
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
           (rois, count, pad(np.asarray(scores, F4)), pad(boxes), pad(kps), pad(np.zeros((n, 3), F4)))]
    out = [torch.full((1,), -7, dtype=torch.int32, device='cuda'), torch.full((K,), -9, dtype=torch.int32, device='cuda'),
           torch.zeros(K, dtype=torch.float32, device='cuda'), torch.zeros((K, 4), dtype=torch.float64, device='cuda'),
           torch.zeros((K, 6, 2), dtype=torch.float64, device='cuda'), torch.zeros((K, 3), dtype=torch.float32, device='cuda')]
    _lib.check(lib.hpe_merge_rois(p(dev[0]), 1, rows, *[p(d) for d in dev[1:]], M, 0, 0, 1, 1, float(F4(iou)), K,
                                  *[p(o) for o in out], None), 'hpe_merge_rois')
    torch.cuda.synchronize()
    kept = int(out[0].cpu()[0])
    assert 0 <= kept <= K
    assert (out[1].cpu().numpy()[kept:] == -9).all()
    return out[1].cpu().numpy()[:kept], out[3].cpu().numpy()[:kept]


@pytest.mark.gpu
def test_gpu_merge_runs_the_same_nms(cases):
    """Fed a frame's thresholded candidates (float64 boxes, the reference's scores, index order) through
    the identity remap, hpe_merge_rois must keep what hpe_detect keeps, in the same order: the two
    callers of the shared sort and greedy pass (csrc/hpe_boxes.h) agree."""
    todo = [('six_frames', f) for f in (0, 3, 4)] + [('flipped', 0), ('zero_area', 0), ('same_box_896', 0),
                                                     ('saturated_high', 0)]
    for name, f in todo:
        c = cases[name]
        fr = c['frames'][f]
        det = gpu_detect([fr], R.logit_threshold(c['t']), c['iou'], c['max_faces'])
        on = R.candidates(fr, c['t'])
        boxes, kps = R.decode(fr['loc'], on)
        src, boxes_out = gpu_merge_identity(R.sigmoid32(fr['cls'][on]), boxes, kps, c['iou'], c['max_faces'], 14, 64)
        n = len(src)
        assert n == int(det['count'][0]), name
        np.testing.assert_array_equal(on[src], det['det_index'][0, :n], err_msg=name)
        assert boxes_out.tobytes() == det['boxes'][0, :n].tobytes(), name


@pytest.mark.gpu
def test_gpu_merge_iou_at_the_threshold(pairs):
    """test_gpu_detect_iou_at_the_threshold and ..._exact_third for hpe_merge_rois: the two boxes of a
    pair, decoded as hpe_detect decodes them, go through the identity remap.  With the threshold on the
    pair's own IoU both are kept, one float32 below it only the first.  (An IoU with the multiply fused
    into the subtraction fails one of the two for every searched pair.)"""
    higher, lower = pairs
    todo = [('higher', R.pair_frame(a, b), 0, 1, ref) for a, b, ref in higher]
    todo += [('lower', R.pair_frame(a, b), 0, 1, ref) for a, b, ref in lower]
    todo += [('third', fr, d0, d1, F4(1 / 3)) for fr, d0, d1 in R.exact_third_frames()]
    failed = []
    for i, (kind, fr, d0, d1, ref) in enumerate(todo):
        on = np.asarray([d0, d1])
        boxes, kps = R.decode(fr['loc'], on)
        sc = R.sigmoid32(fr['cls'][on])
        assert sc[0] > sc[1]
        at = gpu_merge_identity(sc, boxes, kps, ref, 100, 1, 2)[0].tolist()
        below = gpu_merge_identity(sc, boxes, kps, np.nextafter(ref, F4(0)), 100, 1, 2)[0].tolist()
        if at != [0, 1] or below != [0]:
            failed.append((kind, i, float(ref), at, below))
    print('merge, IoU at the threshold: %d of %d pairs fail' % (len(failed), len(todo)))
    assert len(todo) >= 19 and not failed, failed


# ---- GPU: hpe_gather_features ------------------------------------------------------------------------

GATHER_INDEX = (0, 1, 510, 511, 512, 517, 518, 895)
GATHER_COUNT = (8, 1, 2, 3, 5, 8, 4, 1, 0, 6)
GUARD = 64


def _gather_inputs(c0, c1, seed):
    rng = np.random.default_rng(seed)
    n, M = len(GATHER_COUNT), len(GATHER_INDEX)
    det = np.full((n, M), -9, np.int32)
    for i, c in enumerate(GATHER_COUNT):              # frame i starts at index i of the list
        det[i, :c] = np.roll(GATHER_INDEX, -i)[:c]
    return (np.asarray(GATHER_COUNT, np.int32), det, rng.normal(0, 1, (n, 16, 16, c0)).astype(F4),
            rng.normal(0, 1, (n, 8, 8, c1)).astype(F4))


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1, 3, 8])
@pytest.mark.parametrize('c0,c1', [(4, 4), (88, 96), (260, 512)])
def test_gpu_gather_features(c0, c1, k):
    """Hand-made count / det_index: counts of 0, k, below and above k; every index of the list in slot
    0 of some frame; one float4 (c = 4) and a second trip of the 64-lane loop (c > 256); guard words
    after each output."""
    import torch
    lib = _lib.load()
    count, det, tap0, tap1 = _gather_inputs(c0, c1, seed=c0 + k)
    n, M = det.shape
    assert any(c == 0 for c in count) and any(c == k for c in count)
    assert k == M or any(c > k for c in count)          # a count cannot exceed max_faces
    assert k == 1 or any(0 < c < k for c in count)
    dev = [torch.from_numpy(a).cuda() for a in (count, det, tap0, tap1)]
    f0 = torch.full((n * k * c0 + GUARD,), 77.0, dtype=torch.float32, device='cuda')
    f1 = torch.full((n * k * c1 + GUARD,), 77.0, dtype=torch.float32, device='cuda')
    src = torch.full((n * k + GUARD,), -9, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(lib.hpe_gather_features(p(dev[0]), p(dev[1]), n, M, k, p(dev[2]), c0, p(dev[3]), c1, p(f0), p(f1), p(src),
                                       None), 'hpe_gather_features')
    torch.cuda.synchronize()
    f0, f1, src = f0.cpu().numpy(), f1.cpu().numpy(), src.cpu().numpy()
    assert (f0[n * k * c0:] == 77.0).all() and (f1[n * k * c1:] == 77.0).all() and (src[n * k:] == -9).all()
    f0, f1, src = f0[:n * k * c0].reshape(n, k, c0), f1[:n * k * c1].reshape(n, k, c1), src[:n * k].reshape(n, k)
    seen = set()
    for i in range(n):
        w0, w1, ws = D.gather_features(det[i, :count[i]], tap0[i], tap1[i], k)
        assert f0[i].tobytes() == w0.tobytes() and f1[i].tobytes() == w1.tobytes(), i
        np.testing.assert_array_equal(src[i], ws)
        seen |= set(det[i, :min(count[i], k)].tolist())
    assert seen == set(GATHER_INDEX)
