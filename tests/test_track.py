"""Face tracking and pose smoothing across video frames: hpe_track / hpe_track_reset
(csrc/hpe_track.hip), hpe.tracking.PoseTracker and BlazeFaceDetector.detect_video on top.

CPU: the binding, the host-side argument checks, the restatement (tests/track_ref.py) against 19
hpe.detector.EMAFilters and on the issue's hand-made scenario.
GPU: the kernel equals the restatement bit for bit (ids, float64 boxes and keypoints, float32 poses, both
state arrays; output slots at or past a frame's count keep their sentinel), and the Python layers equal
the restatement applied to detect_images' results.

Everything here is exact: there are no tolerances.  What the tracker's defaults do for real video is
unmeasured: the committed data holds no face images."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_ref as TR
from hpe import _lib
from util import fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RID = 'reg1-stoqa9pt-reg2-hrchr82r-selected'
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')
OUT = ('track', 'boxes', 'keypoints', 'poses')


def _bits_equal(got, want, what):
    """Bit for bit, NaN payloads included."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)
    assert not bad.any(), '%s: %d of %d differ, first at %s' % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


# ---- inputs --------------------------------------------------------------------------------------

A, B, C = (.1, .1, .3, .3), (.6, .6, .8, .8), (.1, .6, .3, .8)
SCENARIO = [[A], [A], [B, A], [A, B], [B], [B], [A], [A], [A], [A, B], [C, A, B]]
SCENARIO_IDS = [[0], [0], [1, 0], [0, 1], [1], [1], [0], [0], [0], [0, 2], [-1, 0, 2]]


def _from_boxes(frames, M, seed=0):
    """Per frame a list of boxes -> hpe_track's inputs: seeded keypoints and poses, unused slots poisoned."""
    rng = np.random.default_rng(seed)
    T = len(frames)
    d = dict(count=np.int32([len(f) for f in frames]), boxes=np.full((T, M, 4), 1e300),
             keypoints=np.full((T, M, 6, 2), 1e300), poses=np.full((T, M, 3), np.nan, np.float32))
    for t, f in enumerate(frames):
        for j, b in enumerate(f[:M]):
            d['boxes'][t, j] = b
            d['keypoints'][t, j] = rng.uniform(0, 1, (6, 2))
            d['poses'][t, j] = rng.normal(0, 30, 3).astype(np.float32)
    return d


def _walk(T, M, seed, faces=4, drop=0.15, exact=False):
    """Seeded random walks of 1 .. ``faces`` boxes (exact: ``faces`` of them), each dropping out of a
    frame now and then (if all do, one is kept), in a seeded slot order."""
    rng = np.random.default_rng(seed)
    n = faces if exact else int(rng.integers(1, faces + 1))
    c = rng.uniform(0.2, 0.8, (n, 2))
    hw = rng.uniform(0.04, 0.1, (n, 2))
    frames = []
    for _ in range(T):
        c = c + rng.normal(0, 0.01, (n, 2))
        seen = [i for i in range(n) if rng.uniform() > drop] or [int(rng.integers(n))]
        seen = [seen[i] for i in rng.permutation(len(seen))]
        frames.append([np.concatenate([c[i] - hw[i], c[i] + hw[i]]) for i in seen])
    return _from_boxes(frames, M, seed + 1000)


def _grid(T, M, n, seed):
    """``n`` disjoint boxes per frame on a grid of 10 columns, jittered a little from frame to frame."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(T):
        f = []
        for i in range(n):
            cx, cy = (i % 10 + 0.5) / 10, (i // 10 + 0.5) / 10
            j = rng.normal(0, 0.002, 2)
            f.append((cx - 0.03 + j[0], cy - 0.03 + j[1], cx + 0.03 + j[0], cy + 0.03 + j[1]))
        frames.append(f)
    return _from_boxes(frames, M, seed + 1000)


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _ref(S, d, alpha=0.15, iou=0.3, max_missed=5, K=8, state=None):
    return TR.run(S, d['count'], d['boxes'], d['keypoints'], d['poses'], alpha, iou, max_missed, K, state)


# ---- CPU: binding and host checks ----------------------------------------------------------------

def test_signatures_and_header():
    assert len(_lib.SIGNATURES['hpe_track'][1]) == 18 and len(_lib.SIGNATURES['hpe_track_reset'][1]) == 5
    with open(os.path.join(ROOT, 'include', 'hpe.h')) as fh:
        src = fh.read()
    for name, nargs in (('hpe_track', 18), ('hpe_track_reset', 5)):
        m = re.search(r'^int %s\(([^;]*)\);' % name, src, re.M)
        assert m, name
        assert len(m.group(1).split(',')) == nargs
    assert '#define HPE_TRACK_MAX_TRACKS 64' in src and '#define HPE_TRACK_STATE_D 23' in src
    from hpe import tracking
    assert (tracking.MAX_TRACKS, tracking.STATE_D) == (TR.MAX_TRACKS, TR.STATE_D) == (64, 23)


def _call(lib, p=1, **kw):
    """hpe_track with valid scalars except ``kw``; every pointer is the non-null dummy ``p`` (never
    dereferenced: the host checks come before any device call) or null."""
    a = dict(S=2, T=3, M=4, alpha=0.15, iou=0.3, max_missed=5, K=8)
    a.update(kw)
    q = ctypes.c_void_p(p)
    return lib.hpe_track(a['S'], a['T'], a['M'], q, q, q, q, a['alpha'], a['iou'], a['max_missed'], a['K'], q, q, q,
                         q, q, q, None)


@built
def test_host_checks():
    lib = _lib.load()
    bad = [dict(S=-1), dict(T=-1), dict(M=0), dict(M=-2), dict(K=0), dict(K=65), dict(K=-1), dict(max_missed=-1),
           dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=1.0000001), dict(alpha=float('nan')),
           dict(iou=float('nan')), dict(S=1 << 20, T=1 << 11), dict(S=1 << 40, T=1)]
    for kw in bad:
        assert _call(lib, p=0, **kw) == 1, kw
        assert b'hpe_track' in lib.hpe_last_error(), kw
    assert _call(lib, p=0) == 1 and b'hpe_track: null' in lib.hpe_last_error()
    # S * T == 0: a no-op, also with null pointers; the scalars are still checked
    assert _call(lib, p=0, S=0) == 0 and _call(lib, p=0, T=0) == 0 and _call(lib, p=0, S=0, T=0) == 0
    assert _call(lib, p=0, S=1 << 40, T=0) == 0
    assert _call(lib, p=0, S=0, K=65) == 1
    # one null pointer among valid ones
    q, z = ctypes.c_void_p(1), ctypes.c_void_p(0)
    for i in range(10):
        ptrs = [z if k == i else q for k in range(10)]
        assert lib.hpe_track(1, 1, 1, *ptrs[:4], 0.5, 0.3, 0, 1, *ptrs[4:], None) == 1, i
    # hpe_track_reset
    for S, K in ((-1, 8), (1, 0), (1, 65), (1 << 40, 8)):
        assert lib.hpe_track_reset(S, K, q, q, None) == 1, (S, K)
        assert b'hpe_track_reset' in lib.hpe_last_error()
    assert lib.hpe_track_reset(1, 8, z, q, None) == 1 and lib.hpe_track_reset(1, 8, q, z, None) == 1
    assert b'hpe_track_reset: null' in lib.hpe_last_error()
    assert lib.hpe_track_reset(0, 8, z, z, None) == 0
    assert lib.hpe_track_reset(0, 0, z, z, None) == 1


def test_results_track_field():
    from hpe.detector import Results
    r = Results(np.zeros((2, 4)), np.zeros((2, 6, 2)), np.zeros(2, np.float32), np.zeros((2, 3), np.float32))
    assert r.track.dtype == np.int32 and r.track.tolist() == [-1, -1]
    e = Results(np.zeros((0, 4)), np.zeros((0, 6, 2)), np.zeros(0, np.float32), np.zeros((0, 3), np.float32))
    assert e.track.shape == (0,) and e.track.dtype == np.int32


def test_tracker_argument_errors_without_gpu():
    from hpe.tracking import PoseTracker
    for kw in (dict(streams=0), dict(max_tracks=0), dict(max_tracks=65)):
        with pytest.raises(ValueError):
            PoseTracker(device='cpu', **kw)


# ---- CPU: the restatement ------------------------------------------------------------------------

def test_ref_iou_is_the_detectors():
    from oracle.detector_ref import _iou
    rng = np.random.default_rng(3)
    b = rng.uniform(0, 1, (200, 4)).astype(np.float32)
    b[::7, 2] = b[::7, 0]                                   # zero areas
    for i in range(0, 200, 2):
        _bits_equal(TR.iou(b[i], b[i + 1]), _iou(b[i], b[i + 1]), 'iou')
    assert TR.iou(b[1], b[1]) == 1 and TR.iou(b[7], b[7]) == 0


def _ema_sequence():
    return _walk(12, 3, seed=5, faces=1, drop=0.0)


def test_ref_equals_19_ema_filters():
    """One face, 12 frames, match_iou -1 (the reference's position-only filter): the restatement's
    smoothed values are those of 19 EMAFilters fed the same float64 measurements."""
    from hpe.detector import EMAFilter
    d = _ema_sequence()
    assert d['count'].tolist() == [1] * 12
    tr, bx, kp, ps, si, sd = _ref(1, d, alpha=0.15, iou=-1.0, K=1)
    filt = [EMAFilter(0.15) for _ in range(19)]
    for t in range(12):
        m = np.concatenate([d['boxes'][t, 0], d['keypoints'][t, 0].reshape(12), d['poses'][t, 0].astype(np.float64)])
        s = np.float64([f.update(float(v)) for f, v in zip(filt, m)])
        assert tr[t, 0] == 0
        _bits_equal(np.concatenate([bx[t, 0], kp[t, 0].reshape(12)]), s[:16], 'frame %d' % t)
        _bits_equal(ps[t, 0], s[16:].astype(np.float32), 'pose %d' % t)
    _bits_equal(sd[0, 0, :19], np.float64([f.state for f in filt]), 'state')
    assert si.tolist() == [[1, 0, 0]]
    assert not np.array_equal(bx[5, 0], d['boxes'][5, 0])   # it smooths


def _scenario():
    return _from_boxes(SCENARIO, 3, seed=2)


def test_ref_scenario():
    """An order swap, a 2-frame gap that keeps its id, a 3-frame gap after which the face returns with
    a new id, a detection with no free slot."""
    d = _scenario()
    tr, bx, kp, ps, si, sd = _ref(1, d, iou=0.3, max_missed=2, K=2)
    for t, ids in enumerate(SCENARIO_IDS):
        assert tr[t, :len(ids)].tolist() == ids, t
        assert (tr[t, len(ids):] == TR.SENT_I).all()
        assert (bx[t, len(ids):] == TR.SENT_D).all() and (ps[t, len(ids):] == TR.SENT_F).all()
    assert si[0, 0] == 3 and si[0, 1:3].tolist() == [0, 2]
    # the untracked detection comes back as it went in
    _bits_equal(bx[10, 0], d['boxes'][10, 0], 'untracked box')
    _bits_equal(kp[10, 0], d['keypoints'][10, 0], 'untracked keypoints')
    _bits_equal(ps[10, 0], d['poses'][10, 0], 'untracked pose')
    # a new track's first measurement passes through; a continued one is smoothed
    _bits_equal(bx[2, 0], np.float64(B), 'spawn')
    assert not np.array_equal(kp[3, 0], d['keypoints'][3, 0])


# ---- GPU: the kernel against the restatement -----------------------------------------------------

def _gpu(S, d, alpha=0.15, iou=0.3, max_missed=5, K=8, state=None):
    """hpe_track called directly -> (track, boxes, keypoints, poses, state_i, state_d) on the host.
    state: host (state_i, state_d) to start from; None: hpe_track_reset on sentinel-filled buffers."""
    import torch
    lib = _lib.load()
    n, M = d['boxes'].shape[:2]
    dev = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('count', 'boxes', 'keypoints', 'poses')}
    assert dev['count'].dtype == torch.int32 and dev['boxes'].dtype == torch.float64
    assert dev['poses'].dtype == torch.float32
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    if state is None:
        si = torch.full((S, 1 + 2 * K), 12345, dtype=torch.int32, device='cuda')
        sd = torch.full((S, K, TR.STATE_D), 7.25, dtype=torch.float64, device='cuda')
        _lib.check(lib.hpe_track_reset(S, K, p(si), p(sd), None), 'hpe_track_reset')
    else:
        si, sd = torch.from_numpy(state[0].copy()).cuda(), torch.from_numpy(state[1].copy()).cuda()
    out = [torch.from_numpy(o).cuda() for o in TR.outputs(n, M)]
    _lib.check(lib.hpe_track(S, n // S if S else 0, M, p(dev['count']), p(dev['boxes']), p(dev['keypoints']),
                             p(dev['poses']), alpha, iou, max_missed, K, p(si), p(sd), *[p(o) for o in out], None),
               'hpe_track')
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) + (si.cpu().numpy(), sd.cpu().numpy())


def _same(got, want, what=''):
    for name, g, w in zip(OUT + ('state_i', 'state_d'), got, want):
        _bits_equal(g, w, '%s %s' % (what, name))


def _sentinels_past_count(got, d):
    M = d['boxes'].shape[1]
    for g in range(len(d['count'])):
        c = min(max(int(d['count'][g]), 0), M)
        assert (got[0][g, c:] == TR.SENT_I).all() and (got[1][g, c:] == TR.SENT_D).all()
        assert (got[2][g, c:] == TR.SENT_D).all() and (got[3][g, c:] == TR.SENT_F).all()


@pytest.mark.gpu
def test_gpu_reset():
    import torch
    lib = _lib.load()
    S, K = 3, 5
    si = torch.full((S, 1 + 2 * K), 12345, dtype=torch.int32, device='cuda')
    sd = torch.full((S, K, TR.STATE_D), float('nan'), dtype=torch.float64, device='cuda')
    _lib.check(lib.hpe_track_reset(S, K, ctypes.c_void_p(si.data_ptr()), ctypes.c_void_p(sd.data_ptr()), None), 'reset')
    wi, wd = TR.new_state(S, K)
    _bits_equal(si.cpu().numpy(), wi, 'state_i')
    _bits_equal(sd.cpu().numpy(), wd, 'state_d')


@pytest.mark.gpu
def test_gpu_scenario_and_ema_sequence():
    d = _scenario()
    got = _gpu(1, d, iou=0.3, max_missed=2, K=2)
    _same(got, _ref(1, d, iou=0.3, max_missed=2, K=2), 'scenario')
    _sentinels_past_count(got, d)
    assert [got[0][t, :len(i)].tolist() for t, i in enumerate(SCENARIO_IDS)] == SCENARIO_IDS and got[4][0, 0] == 3
    e = _ema_sequence()
    _same(_gpu(1, e, iou=-1.0, K=1), _ref(1, e, iou=-1.0, K=1), 'ema')


@pytest.mark.gpu
def test_gpu_chunks_carry_the_state():
    d = _walk(11, 6, seed=21)
    whole = _gpu(1, d, max_missed=1, K=4)
    _same(whole, _ref(1, d, max_missed=1, K=4), 'whole')
    state, parts = None, []
    for lo, hi in ((0, 5), (5, 10), (10, 11)):
        r = _gpu(1, {k: v[lo:hi] for k, v in d.items()}, max_missed=1, K=4, state=state)
        state = r[4:]
        parts.append(r[:4])
    for i, name in enumerate(OUT):
        _bits_equal(np.concatenate([p[i] for p in parts]), whole[i], name)
    _bits_equal(state[0], whole[4], 'state_i')
    _bits_equal(state[1], whole[5], 'state_d')


@pytest.mark.gpu
def test_gpu_streams_do_not_leak():
    ds = [_walk(9, 5, seed=s) for s in (31, 32, 33)]
    got = _gpu(3, _cat(ds), max_missed=2, K=3)
    _same(got, _ref(3, _cat(ds), max_missed=2, K=3), 'S=3')
    for s, d in enumerate(ds):
        one = _gpu(1, d, max_missed=2, K=3)
        for i, name in enumerate(OUT):
            _bits_equal(got[i][s * 9:(s + 1) * 9], one[i], '%s of stream %d' % (name, s))
        _bits_equal(got[4][s:s + 1], one[4], 'state_i')
        _bits_equal(got[5][s:s + 1], one[5], 'state_d')
    assert len({g.tobytes() for g in got[5]}) == 3


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 64])
def test_gpu_slots_fill_and_overflow(K):
    d = _grid(3, 100, 70, seed=41)
    assert d['count'].tolist() == [70] * 3
    got = _gpu(1, d, K=K)
    _same(got, _ref(1, d, K=K), 'K=%d' % K)
    _sentinels_past_count(got, d)
    assert (got[0][:, :K] >= 0).all() and (got[0][:, K:70] == -1).all()
    _bits_equal(got[1][:, K:70], d['boxes'][:, K:70], 'untracked boxes')
    _bits_equal(got[3][:, K:70], d['poses'][:, K:70], 'untracked poses')


@pytest.mark.gpu
@pytest.mark.parametrize('T,M,K', [(10, 1, 2), (1, 4, 8), (1, 1, 1), (13, 5, 64), (13, 5, 1)])
def test_gpu_shapes(T, M, K):
    d = _walk(T, M, seed=50 + T + M)
    got = _gpu(1, d, max_missed=1, K=K)
    _same(got, _ref(1, d, max_missed=1, K=K), 'T=%d M=%d K=%d' % (T, M, K))
    _sentinels_past_count(got, d)


@pytest.mark.gpu
def test_gpu_count_cases():
    d = _walk(8, 3, seed=61, faces=3, drop=0.0, exact=True)
    assert d['count'].tolist() == [3] * 8    # every slot of every frame holds a detection
    d['count'][2] = -3           # clamped to 0: an empty frame
    d['count'][4] = 0            # a frame without faces between frames with faces
    d['count'][6] = 3 + 5        # clamped to M
    got = _gpu(1, d, max_missed=3, K=4)
    _same(got, _ref(1, d, max_missed=3, K=4), 'counts')
    _sentinels_past_count(got, d)
    assert (got[0][2] == TR.SENT_I).all() and (got[0][4] == TR.SENT_I).all() and (got[0][6] != TR.SENT_I).all()


@pytest.mark.gpu
def test_gpu_identical_boxes_tie_to_lowest_slot():
    d = _from_boxes([[A, A], [A]], 2, seed=7)
    got = _gpu(1, d, K=4)
    _same(got, _ref(1, d, K=4), 'tie')
    assert got[0][0].tolist() == [0, 1] and got[0][1, 0] == 0
    assert got[4][0].tolist() == [2, 0, 1, -1, -1, 0, 1, 0, 0]   # next_id, ids, misses: track 1 missed once


@pytest.mark.gpu
def test_gpu_non_finite_boxes_are_passed_by():
    d = _from_boxes([[A, B], [A, B, C], [A, B]], 3, seed=8)
    nan = np.uint64(0x7ff800000000beef).view(np.float64)
    d['boxes'][1, 0, 2] = nan                 # A in frame 1: a NaN with a payload
    d['boxes'][1, 2, 1] = np.inf              # C in frame 1
    d['boxes'][2, 1, 0] = -np.inf             # B in frame 2
    got = _gpu(1, d, K=4)
    _same(got, _ref(1, d, K=4), 'non-finite')
    assert got[0][:, :].tolist() == [[0, 1, TR.SENT_I], [-1, 1, -1], [0, -1, TR.SENT_I]]
    for t, j in ((1, 0), (1, 2), (2, 1)):
        _bits_equal(got[1][t, j], d['boxes'][t, j], 'box')
        _bits_equal(got[2][t, j], d['keypoints'][t, j], 'keypoints')
        _bits_equal(got[3][t, j], d['poses'][t, j], 'pose')
    # the state is what the same frames without those detections leave
    e = _from_boxes([[A, B], [B], [A]], 3, seed=8)
    for k in ('boxes', 'keypoints', 'poses'):
        e[k][1, 0], e[k][2, 0] = d[k][1, 1], d[k][2, 0]
    clean = _gpu(1, e, K=4)
    _bits_equal(got[4], clean[4], 'state_i')
    _bits_equal(got[5], clean[5], 'state_d')


@pytest.mark.gpu
def test_gpu_zero_area_box():
    Z = (.4, .4, .4, .6)
    d = _from_boxes([[Z], [Z], [Z]], 1, seed=9)
    spawn = _gpu(1, d, iou=0.3, K=4)
    _same(spawn, _ref(1, d, iou=0.3, K=4), 'zero area, 0.3')
    assert spawn[0][:, 0].tolist() == [0, 1, 2]
    match = _gpu(1, d, iou=-1.0, K=4)
    _same(match, _ref(1, d, iou=-1.0, K=4), 'zero area, -1')
    assert match[0][:, 0].tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_gpu_iou_at_the_threshold():
    """Box pairs whose IoU a fused multiply-add in the denominator moves by one float32
    (tests/detect_ref.py's seeded search; tests/test_detect_kernel.py holds on the CPU that it yields
    them): frame 0 holds the pair's first box, frame 1 its second.  With match_iou on the pair's own IoU
    frame 1 starts track 1, one float32 below it frame 1 continues track 0; outputs and state equal the
    restatement bit for bit.  (A contracted IoU fails one of the two for every pair.)"""
    import detect_ref as R
    higher, lower = R.iou_pairs()
    assert len(higher) >= 8 and len(lower) >= 8
    for kind, group in (('higher', higher), ('lower', lower)):
        for i, (a, b, ref) in enumerate(group):
            boxes, _ = R.decode(R.pair_frame(a, b)['loc'], np.arange(2))
            assert R.iou(boxes[0].astype(np.float32), boxes[1].astype(np.float32)).tobytes() == ref.tobytes()
            d = _from_boxes([[boxes[0]], [boxes[1]]], 1, seed=11)
            for thr, ids in ((ref, [0, 1]), (np.nextafter(ref, np.float32(0)), [0, 0])):
                got = _gpu(1, d, iou=float(thr), K=2)
                _same(got, _ref(1, d, iou=float(thr), K=2), '%s pair %d at %r' % (kind, i, thr))
                assert got[0][:, 0].tolist() == ids, (kind, i, float(ref), float(thr), got[0][:, 0].tolist())


@pytest.mark.gpu
def test_gpu_alpha_one_copies():
    d = _walk(9, 4, seed=71, drop=0.1)
    got = _gpu(1, d, alpha=1.0, K=8)
    _same(got, _ref(1, d, alpha=1.0, K=8), 'alpha 1')
    n = 0
    for t in range(9):
        for j in range(int(d['count'][t])):
            assert got[0][t, j] >= 0
            _bits_equal(got[1][t, j], d['boxes'][t, j], 'box')
            _bits_equal(got[2][t, j], d['keypoints'][t, j], 'keypoints')
            _bits_equal(got[3][t, j], d['poses'][t, j], 'pose')
            n += 1
    assert n > 9


@pytest.mark.gpu
def test_gpu_next_id_wraps():
    d = _from_boxes([[A, B, C]], 3, seed=10)
    si, sd = TR.new_state(1, 4)
    si[0, 0] = 0x7fffffff
    got = _gpu(1, d, K=4, state=(si, sd))
    _same(got, _ref(1, d, K=4, state=(si, sd)), 'wrap')
    assert got[0][0].tolist() == [0x7fffffff, 0, 1] and got[4][0, 0] == 2


# ---- GPU: through Python -------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_pose_tracker_update():
    import torch
    from hpe.tracking import PoseTracker
    ds = [_walk(7, 5, seed=s) for s in (81, 82)]
    d = _cat(ds)
    scores = np.random.default_rng(1).uniform(0, 1, (14, 5)).astype(np.float32)
    r = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    r['scores'] = torch.from_numpy(scores).cuda()
    r['det_index'] = torch.zeros((14, 5), dtype=torch.int32, device='cuda')
    trk = PoseTracker(alpha=0.3, match_iou=0.2, max_missed=1, max_tracks=3, streams=2)
    si, sd = trk.state()
    _bits_equal(si, TR.new_state(2, 3)[0], 'fresh state_i')
    _bits_equal(sd, TR.new_state(2, 3)[1], 'fresh state_d')
    out = trk.update(r)
    assert set(out) == {'count', 'scores', 'track', 'boxes', 'keypoints', 'poses'}
    assert all(v.is_cuda for v in out.values()) and out['track'].dtype == torch.int32
    assert out['count'] is r['count'] and out['scores'] is r['scores']
    want = _ref(2, d, alpha=0.3, iou=0.2, max_missed=1, K=3)
    for g in range(14):
        c = int(d['count'][g])
        for i, name in enumerate(OUT):
            _bits_equal(out[name][g, :c].cpu().numpy(), want[i][g, :c], name)
    si, sd = trk.state()
    _bits_equal(si, want[4], 'state_i')
    _bits_equal(sd, want[5], 'state_d')
    trk.reset()
    _bits_equal(trk.state()[0], TR.new_state(2, 3)[0], 'reset')
    with pytest.raises(ValueError):
        trk.update({k: v[:13] for k, v in r.items()})
    with pytest.raises(ValueError):
        PoseTracker(alpha=0.0).update(r)


M_FACES = 8
REPEAT = 4


@pytest.fixture(scope='module')
def video():
    """The seeded noise frames of tests/test_rois.py / tests/test_tiled.py, each repeated 4 times, and
    detect_images' results for them; computed once."""
    from hpe.detector import BlazeFaceDetector
    u8 = np.random.default_rng(11).integers(0, 256, (4, 96, 160, 3), dtype=np.uint8)
    mc, w = fixture(RID)
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.15, max_faces=M_FACES)
    clips = np.repeat(u8[:, None], REPEAT, axis=1)                      # (4, 4, 96, 160, 3)
    per = [det.detect_images(c, crop='square') for c in clips]
    return dict(det=det, u8=u8, clips=clips, per=per)


def _pack(results, M):
    p = dict(count=np.int32([len(r.scores) for r in results]), boxes=np.full((len(results), M, 4), 1e300),
             keypoints=np.full((len(results), M, 6, 2), 1e300), poses=np.full((len(results), M, 3), np.nan, np.float32))
    for i, r in enumerate(results):
        for k in ('boxes', 'keypoints', 'poses'):
            p[k][i, :len(r.scores)] = getattr(r, k)
    return p


def _results_equal(res, want, g0, what):
    """[Results] of frames g0 .. against the restatement's outputs."""
    for t, r in enumerate(res):
        c = len(r.scores)
        for i, name in enumerate(OUT):
            _bits_equal(getattr(r, name), want[i][g0 + t, :c], '%s %s frame %d' % (what, name, t))


@pytest.mark.gpu
def test_gpu_detect_video(video):
    from hpe.tracking import PoseTracker
    det = video['det']
    positive = 0
    for s, (clip, per) in enumerate(zip(video['clips'], video['per'])):
        d = _pack(per, M_FACES)
        assert d['count'].min() >= 1 and len(set(d['count'].tolist())) == 1
        want = _ref(1, d)
        trk = PoseTracker(device=det.device)
        res = det.detect_video(clip, trk, crop='square')
        assert len(res) == REPEAT
        _results_equal(res, want, 0, 'clip %d' % s)
        for r, p in zip(res, per):
            _bits_equal(r.scores, p.scores, 'scores')
            assert r.track.dtype == np.int32 and r.track.shape == r.scores.shape
        _bits_equal(trk.state()[0], want[4], 'state_i')
        _bits_equal(trk.state()[1], want[5], 'state_d')
        # identical boxes have IoU 1: a positive-area face keeps its id over the repeats
        b = per[0].boxes.astype(np.float32)
        pos = (np.abs(b[:, 2] - b[:, 0]) * np.abs(b[:, 3] - b[:, 1])) > 0
        positive += int(pos.sum())
        for r in res[1:]:
            assert (r.track[pos] == res[0].track[pos]).all() and (r.track[pos] >= 0).all()
        # frames [:2] then [2:] continue the same video
        trk2 = PoseTracker(device=det.device)
        halves = det.detect_video(clip[:2], trk2, crop='square') + det.detect_video(clip[2:], trk2, crop='square')
        _results_equal(halves, want, 0, 'halves of clip %d' % s)
        _bits_equal(trk2.state()[1], want[5], 'state_d of the halves')
    assert positive >= 1
    assert det.detect_video(video['clips'][0][:0], PoseTracker(device=det.device)) == []


@pytest.mark.gpu
def test_gpu_detect_video_streams(video):
    from hpe.tracking import PoseTracker
    det = video['det']
    trk = PoseTracker(streams=4, device=det.device)
    res = det.detect_video(video['clips'], trk, crop='square')
    assert len(res) == 4 and all(len(r) == REPEAT for r in res)
    si, sd = trk.state()
    for s, per in enumerate(video['per']):
        want = _ref(1, _pack(per, M_FACES))
        _results_equal(res[s], want, 0, 'stream %d' % s)
        _bits_equal(si[s:s + 1], want[4], 'state_i')
        _bits_equal(sd[s:s + 1], want[5], 'state_d')
    with pytest.raises(ValueError):
        det.detect_video(video['clips'][:3], trk, crop='square')
    with pytest.raises(ValueError):
        det.detect_video(video['clips'][0], trk, crop='square')


@pytest.mark.gpu
def test_gpu_tracker_on_merged_tiles(video):
    """tracker.update on merge_rois' dict, whose slot count (32) is not the detector's max_faces (8)."""
    import torch
    from hpe.preprocess import prepare_rois, tile_rois
    from hpe.tracking import PoseTracker
    det = video['det']
    frames = np.repeat(video['u8'][:2], 3, axis=0)                      # 2 streams x 3 frames, stream-major
    rois, per = tile_rois(6, 96, 160, 64, 16)
    t = torch.from_numpy(rois).to(det.device)
    r = det.postprocess(det.net.forward(prepare_rois(frames, t, device=det.device)))
    merged = det.merge_rois(r, t, per, (0, 0, 160, 96), max_faces=32)
    trk = PoseTracker(max_tracks=16, streams=2, device=det.device)
    out = trk.update(merged)
    h = {k: v.cpu().numpy() for k, v in merged.items()}
    assert h['boxes'].shape == (6, 32, 4) and h['count'].min() >= 1
    want = _ref(2, h, K=16)
    for g in range(6):
        c = int(h['count'][g])
        for i, name in enumerate(OUT):
            _bits_equal(out[name][g, :c].cpu().numpy(), want[i][g, :c], name)
    _bits_equal(trk.state()[0], want[4], 'state_i')
    _bits_equal(trk.state()[1], want[5], 'state_d')
