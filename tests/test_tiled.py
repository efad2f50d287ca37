"""Tiled detection: hpe.preprocess.tile_rois (the host table), hpe_merge_rois (csrc/hpe_merge.hip) and
BlazeFaceDetector.merge_rois / detect_tiled on top.

CPU: the table's geometry over a sweep of (L, tile, overlap) and against the restatement
(tests/merge_ref.py); the binding; the host-side argument checks; Results' new fields.
GPU: the kernel equals the restatement bit for bit on hand-made per-ROI results (count, src, scores,
poses, float64 boxes and keypoints; the slots past the count untouched), and detect_tiled equals its
parts composed by hand.

Detection quality of any tile / overlap is unmeasured: the committed data holds no face images."""
import ctypes
import os

import numpy as np
import pytest

import merge_ref as MR
import roi_ref as R
from hpe import _lib
from util import fixture

RID = 'reg1-stoqa9pt-reg2-hrchr82r-selected'
built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libhpe.so not built')
FIELDS = ('boxes', 'keypoints', 'scores', 'poses')


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the tile table ------------------------------------------------------------------------------

def test_tile_offsets_geometry_sweep():
    from hpe.preprocess import tile_offsets
    seen_many = 0
    for tile in range(1, 17):
        for overlap in range(tile):
            for L in range(1, 70):
                off = tile_offsets(L, tile, overlap)
                assert off == MR.offsets(L, tile, overlap)
                if L <= tile:                        # one centred tile, its outside padded
                    assert off == [-((tile - L) // 2)]
                    assert off[0] <= 0 and off[0] + tile >= L
                    assert abs((-off[0]) - (off[0] + tile - L)) <= 1
                    continue
                assert off[0] == 0 and off[-1] + tile == L
                assert len(off) == -(-(L - tile) // (tile - overlap)) + 1
                d = np.diff(off)
                assert (d >= 1).all() and (d <= tile - overlap).all()   # neighbours share >= overlap pixels
                covered = np.zeros(L, bool)
                for o in off:
                    covered[o:o + tile] = True
                assert covered.all()
                seen_many += len(off) > 2
    assert seen_many > 1000


@pytest.mark.parametrize('crop', [None, 'square', (10, 5, 100, 37)])
@pytest.mark.parametrize('full', [True, False])
def test_tile_rois_rows(crop, full):
    from hpe.preprocess import crop_rect, tile_offsets, tile_rois
    h, w, tile, overlap = 96, 160, 40, 12
    rois, per = tile_rois(3, h, w, tile, overlap, crop=crop, full=full)
    want, wper = MR.tile_rois(3, h, w, tile, overlap, crop=crop, full=full)
    assert rois.dtype == np.int32 and rois.shape == (3 * per, 5) and per == wper
    np.testing.assert_array_equal(rois, want)
    sx, sy, sw, sh = crop_rect(h, w, crop)
    ox, oy = tile_offsets(sw, tile, overlap), tile_offsets(sh, tile, overlap)
    assert per == len(ox) * len(oy) + full
    for f in range(3):                                # frame-major, row 0 the whole look, y outer, x inner
        rows = rois[f * per:(f + 1) * per]
        assert (rows[:, 0] == f).all()
        if full:
            np.testing.assert_array_equal(rows[0, 1:], (sx, sy, sw, sh))
        tiles = rows[full:]
        np.testing.assert_array_equal(tiles[:, 1], np.tile(np.add(ox, sx), len(oy)))
        np.testing.assert_array_equal(tiles[:, 2], np.repeat(np.add(oy, sy), len(ox)))
        assert (tiles[:, 3:] == tile).all()
    assert all(R.valid(r, 3) for r in rois)
    if crop == 'square':
        assert (sx, sy, sw, sh) == (32, 0, 96, 96)


def test_tile_rois_small_axis_none_and_errors():
    from hpe.preprocess import tile_rois
    # L <= tile on both axes: one centred tile reaching outside the frame
    rois, per = tile_rois(2, 10, 20, 32, 8)
    assert per == 2
    np.testing.assert_array_equal(rois, [(0, 0, 0, 20, 10), (0, -6, -11, 32, 32), (1, 0, 0, 20, 10),
                                         (1, -6, -11, 32, 32)])
    assert all(R.valid(r, 2) for r in rois)
    # the issue's benchmark shape: 7 x 4 tiles and the whole look
    assert tile_rois(1, 720, 1280, 256, 64)[1] == 29
    # tile=None: the whole look only
    rois, per = tile_rois(2, 96, 160, None, None, crop='square')
    assert per == 1
    np.testing.assert_array_equal(rois, [(0, 32, 0, 96, 96), (1, 32, 0, 96, 96)])
    rois, per = tile_rois(0, 96, 160, 64, 16)
    assert rois.shape == (0, 5) and rois.dtype == np.int32 and per == 7
    for kw in (dict(tile=0, overlap=0), dict(tile=-3, overlap=0), dict(tile=8, overlap=8), dict(tile=8, overlap=-1),
               dict(tile=None, overlap=0, full=False)):
        with pytest.raises(ValueError):
            tile_rois(1, 96, 160, **kw)


# ---- interface, no device ----------------------------------------------------------------------

def test_signature_is_bound():
    res, args = _lib.SIGNATURES['hpe_merge_rois']
    assert res is ctypes.c_int and len(args) == 22
    assert args[1] is ctypes.c_int64 and args[13] is ctypes.c_float
    assert [i for i, a in enumerate(args) if a is ctypes.c_int32] == [2, 8, 9, 10, 11, 12, 14]


@built
def test_hpe_merge_rois_rejects_bad_arguments():
    lib = _lib.load()
    z = ctypes.c_void_p(256)
    names = ('rois', 'count', 'scores', 'boxes', 'keypoints', 'poses', 'count_out', 'src_out', 'scores_out',
             'boxes_out', 'keypoints_out', 'poses_out')

    def call(n=1, rows=2, m_in=4, dst=(0, 0, 8, 8), m_out=4, **ptrs):
        p = {k: ptrs.get(k, z) for k in names}
        return lib.hpe_merge_rois(p['rois'], n, rows, p['count'], p['scores'], p['boxes'], p['keypoints'], p['poses'],
                                  m_in, dst[0], dst[1], dst[2], dst[3], 0.3, m_out, p['count_out'], p['src_out'],
                                  p['scores_out'], p['boxes_out'], p['keypoints_out'], p['poses_out'], None)

    def rejected(**kw):
        rc = call(**kw)
        return rc == 1 and b'hpe_merge_rois' in lib.hpe_last_error()

    for k in names:
        assert rejected(**{k: None}), k
        assert b'null' in lib.hpe_last_error()
    assert rejected(n=-1)
    assert b'negative' in lib.hpe_last_error()
    for kw in (dict(rows=0), dict(rows=-2), dict(m_in=0), dict(m_out=0), dict(m_out=-1), dict(dst=(0, 0, 0, 8)),
               dict(dst=(0, 0, 8, -1))):
        assert rejected(**kw), kw
        assert b'positive' in lib.hpe_last_error()
    L = 1 << 24
    for dst in ((L + 1, 0, 8, 8), (-L - 1, 0, 8, 8), (0, L + 1, 8, 8), (0, -L - 1, 8, 8), (0, 0, L + 1, 8),
                (0, 0, 8, L + 1)):
        assert rejected(dst=dst), dst
        assert b'2^24' in lib.hpe_last_error()
    assert rejected(n=1 << 31)
    assert rejected(n=1 << 40)
    assert b'too large' in lib.hpe_last_error()
    assert rejected(rows=64, m_in=65)
    assert b'HPE_MERGE_MAX_CAND' in lib.hpe_last_error()
    assert rejected(rows=1 << 30, m_in=1 << 30)
    assert rejected(rows=4097, m_in=1)
    # no frames: a no-op, also without buffers
    assert call(n=0) == 0
    assert call(n=0, **{k: None for k in names}) == 0
    assert rejected(n=0, rows=0)


def test_results_roi_default():
    from hpe.detector import Results
    r = Results(np.zeros((2, 4)), np.zeros((2, 6, 2)), np.zeros(2, np.float32), np.zeros((2, 3), np.float32))
    for a in (r.roi, r.src):
        assert a.dtype == np.int32 and a.shape == (2,) and not a.any()
    e = Results(np.zeros((0, 4)), np.zeros((0, 6, 2)), np.zeros(0, np.float32), np.zeros((0, 3), np.float32))
    assert e.roi.shape == (0,) and e.roi.dtype == np.int32


# ---- hpe_merge_rois against the restatement ------------------------------------------------------

DST = (0, 0, 160, 96)


def _inputs(n, rows, M, seed, dst=DST, clusters=12, half=0.05, counts=None):
    """Hand-made per-ROI results: per frame a non-square row 0 (dst itself) and square rows around it,
    some starting at negative coordinates; boxes that land, after the remap, near one of ``clusters``
    centres of the destination (so that the NMS has work to do); scores from 63 values (many ties)."""
    rng = np.random.default_rng(seed)
    rois = np.zeros((n, rows, 5), np.int64)
    rois[:, :, 0] = np.arange(n)[:, None]
    side = rng.integers(32, 81, (n, rows))
    rois[:, :, 1] = dst[0] + rng.integers(-20, dst[2] - 20, (n, rows))
    rois[:, :, 2] = dst[1] + rng.integers(-20, dst[3] - 20, (n, rows))
    rois[:, :, 3] = rois[:, :, 4] = side
    rois[:, 0, 1:] = dst
    rois = rois.reshape(-1, 5).astype(np.int32)
    m = n * rows
    count = rng.integers(0, M + 1, m).astype(np.int32) if counts is None else np.asarray(counts, np.int32)
    centres = rng.uniform(0.1, 0.9, (clusters, 2))
    c = centres[rng.integers(0, clusters, (m, M))] + rng.normal(0, 0.004, (m, M, 2))
    hw = half + rng.uniform(0, half / 2, (m, M, 2))

    def inverse(p):                                  # destination-normalised -> ROI-normalised (roughly)
        o = np.array(dst[:2], np.float64)
        s = np.array(dst[2:], np.float64)
        return (p * s + o - rois[:, None, None, 1:3]) / rois[:, None, None, 3:5]

    boxes = inverse(np.stack([c - hw, c + hw], 2)).reshape(m, M, 4)
    kps = inverse(rng.uniform(0, 1, (m, M, 6, 2)))
    scores = (rng.integers(1, 64, (m, M)) / 64.0).astype(np.float32)
    poses = rng.normal(0, 30, (m, M, 3)).astype(np.float32)
    return dict(rois=rois, rows=rows, count=count, scores=scores, boxes=np.ascontiguousarray(boxes),
                keypoints=np.ascontiguousarray(kps), poses=poses, dst=dst, iou=0.3, K=100)


def _full_counts(total, rows, M):
    """`total` candidates over rows of M slots: full rows, one partial row, empty rows."""
    assert total <= rows * M
    return [min(max(total - r * M, 0), M) for r in range(rows)]


def _gpu_merge(c):
    import torch
    lib = _lib.load()
    m, M = c['scores'].shape
    n, K = m // c['rows'], c['K']
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
           for k in ('rois', 'count', 'scores', 'boxes', 'keypoints', 'poses')}
    assert dev['rois'].dtype == torch.int32 and dev['boxes'].dtype == torch.float64
    out = dict(count=torch.full((n,), -7, dtype=torch.int32, device='cuda'),
               src=torch.full((n, K), -9, dtype=torch.int32, device='cuda'),
               scores=torch.full((n, K), 77.0, dtype=torch.float32, device='cuda'),
               boxes=torch.full((n, K, 4), 1e300, dtype=torch.float64, device='cuda'),
               keypoints=torch.full((n, K, 6, 2), 1e300, dtype=torch.float64, device='cuda'),
               poses=torch.full((n, K, 3), 77.0, dtype=torch.float32, device='cuda'))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    d = c['dst']
    _lib.check(lib.hpe_merge_rois(p(dev['rois']), n, c['rows'], p(dev['count']), p(dev['scores']), p(dev['boxes']),
                                  p(dev['keypoints']), p(dev['poses']), M, d[0], d[1], d[2], d[3], c['iou'], K,
                                  p(out['count']), p(out['src']), p(out['scores']), p(out['boxes']),
                                  p(out['keypoints']), p(out['poses']), None), 'hpe_merge_rois')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits_equal(got, want, what):
    """Bit for bit; a NaN must be a NaN in the same place (its payload is the hardware's)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want) if got.dtype.kind == 'f' else np.zeros(want.shape, bool)
    if got.dtype.kind == 'f':
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(u)[~nan], np.ascontiguousarray(want).view(u)[~nan],
                                  err_msg=what)


SENTINEL = dict(src=-9, scores=77.0, boxes=1e300, keypoints=1e300, poses=77.0)


def _check(c):
    """The kernel on case c equals the restatement; returns the restatement's per-frame dicts."""
    want = MR.merge(c['rois'], c['rows'], c['count'], c['scores'], c['boxes'], c['keypoints'], c['poses'], c['dst'],
                    c['iou'], c['K'])
    got = _gpu_merge(c)
    np.testing.assert_array_equal(got['count'], [len(w['src']) for w in want])
    for f, w in enumerate(want):
        k = len(w['src'])
        for key in ('src', 'scores', 'poses', 'boxes', 'keypoints'):
            _bits_equal(got[key][f, :k], w[key], '%s of frame %d' % (key, f))
            assert (got[key][f, k:] == SENTINEL[key]).all(), 'slots past the count were written: %s' % key
    return want


def _offered(c, f):
    """Candidates frame f's rows offer, before validity and the drop rules."""
    M = c['scores'].shape[1]
    return int(np.clip(c['count'][f * c['rows']:(f + 1) * c['rows']], 0, M).sum())


@pytest.mark.gpu
def test_gpu_merge_no_candidates_and_one():
    c = _inputs(2, 3, 4, seed=1, counts=[0] * 6)
    assert [len(w['src']) for w in _check(c)] == [0, 0]
    c['count'][4] = 1                                   # frame 1, row 1, slot 0
    want = _check(c)
    assert len(want[0]['src']) == 0 and want[1]['src'].tolist() == [4]


@pytest.mark.gpu
@pytest.mark.parametrize('M', [1, 5])
def test_gpu_merge_one_row_per_frame(M):
    want = _check(_inputs(3, 1, M, seed=2, counts=[M, 0, M]))
    assert len(want[0]['src']) >= 1 and len(want[1]['src']) == 0


@pytest.mark.gpu
def test_gpu_merge_row_validity_and_counts():
    c = _inputs(3, 4, 6, seed=3, counts=[6] * 12, clusters=40, half=0.02)
    c['rois'][1] = R.INVALID                            # a filler between valid rows
    c['rois'][4 + 2, 0] = 0                             # frame 1's row 2 names frame 0
    c['rois'][8 + 1, 3] = 0                             # zero width
    c['rois'][8 + 3, 1] = (1 << 24) + 1                 # x0 beyond the bound
    c['count'][0] = 9                                   # above M: clamped
    c['count'][3] = -2                                  # negative: nothing
    c['count'][8] = 2 ** 31 - 1
    want = _check(c)
    rows = [set((w['src'] // 6).tolist()) for w in want]
    assert rows[0] <= {0, 2} and rows[1] <= {0, 1, 3} and rows[2] <= {0, 2}
    assert all(len(r) >= 2 for r in rows)


@pytest.mark.gpu
def test_gpu_merge_score_ties_across_rows():
    """Every score equal and every row holding the same boxes: of each group of duplicates the lowest
    r * M + j survives, so every survivor comes from row 0."""
    c = _inputs(2, 5, 4, seed=4, counts=[4] * 10, clusters=4)
    c['scores'][:] = np.float32(0.625)
    c['rois'][:, 1:] = DST
    c['boxes'][:] = c['boxes'][0]
    want = _check(c)
    for w in want:
        assert len(w['src']) >= 1 and (w['src'] < 4).all() and (np.diff(w['src']) > 0).all()
    # ties between different boxes: the generator's 63 score values over 40 candidates per frame
    c = _inputs(2, 5, 8, seed=5, counts=[8] * 10, clusters=30, half=0.02)
    want = _check(c)
    assert any(len(set(w['scores'].tolist())) < len(w['scores']) for w in want)


@pytest.mark.gpu
def test_gpu_merge_degenerate_boxes():
    c = _inputs(1, 3, 6, seed=6, counts=[6] * 3, clusters=3)
    c['rois'][:, 1:] = DST                              # one geometry: a copied box lands where it was
    b, s = c['boxes'], c['scores']
    s[:] = np.linspace(0.9, 0.1, 18, dtype=np.float32).reshape(3, 6)
    b[0, 1, 2] = b[0, 1, 0]                             # zero width: IoU 0, never suppressed, suppresses nothing
    b[0, 2] = b[0, 0]
    b[0, 2, 3] = b[0, 2, 1]                             # zero height on top of the best box
    b[1, 0] = b[0, 0][[2, 3, 0, 1]]                     # the best box with swapped corners: suppressed
    b[1, 1] = b[1, 1][[2, 1, 0, 3]]                     # x corners swapped only
    b[1, 2, 0] = np.nan                                 # dropped
    b[1, 3, 3] = np.inf                                 # dropped
    b[2, 0, 1] = -np.inf                                # dropped
    s[2, 1] = np.nan                                    # dropped
    c['keypoints'][0, 0, 2, 1] = np.nan                 # a kept box (the top score): passed through
    c['keypoints'][0, 0, 4, 0] = np.inf
    want = _check(c)[0]
    src = want['src'].tolist()
    assert src[0] == 0 and 1 in src and 2 in src and 6 not in src
    assert not {8, 9, 12, 13} & set(src)
    assert np.isnan(want['keypoints'][0, 2, 1]) and np.isinf(want['keypoints'][0, 4, 0])
    assert np.isfinite(want['boxes']).all()


@pytest.mark.gpu
def test_gpu_merge_output_cap():
    c = _inputs(2, 4, 8, seed=7, counts=[8] * 8, clusters=60, half=0.01)
    uncapped = _check(c)
    assert all(len(w['src']) > 5 for w in uncapped)
    c['K'] = 5
    capped = _check(c)
    for a, b in zip(capped, uncapped):
        assert a['src'].tolist() == b['src'][:5].tolist()
    c['K'] = 1
    _check(c)


@pytest.mark.gpu
@pytest.mark.parametrize('dst', [DST, (-7, -3, 160, 96), (13, 9, 51, 77)])
def test_gpu_merge_remap_geometry(dst):
    """Row 0 is the non-square destination itself, the other rows squares, some at negative origins."""
    c = _inputs(2, 6, 4, seed=8, dst=dst, clusters=20, half=0.03)
    assert (c['rois'][:, 1] < 0).any() and (c['rois'][:, 2] < 0).any()
    assert c['rois'][0, 3] != c['rois'][0, 4]
    want = _check(c)
    assert all(len(set((w['src'] // 4).tolist())) >= 2 for w in want)
    # row 0 maps onto itself up to the rounding of the identity
    row0 = [i for i, s in enumerate(want[0]['src']) if s < 4]
    assert row0
    for i in row0:
        np.testing.assert_allclose(want[0]['boxes'][i], c['boxes'][0, want[0]['src'][i]], rtol=0, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('total', [255, 256, 257, 1025, 4096])
def test_gpu_merge_candidate_counts(total):
    """Around the workgroup's 256 threads and around powers of two (the sort's size), up to the cap
    (64 rows x 64 slots); frame 1 holds three candidates fewer, so both sides of each size are run."""
    rows, M = -(-total // 64), 64
    counts = _full_counts(total, rows, M) + _full_counts(total - 3, rows, M)
    c = _inputs(2, rows, M, seed=total, counts=counts, clusters=14)
    assert _offered(c, 0) == total and _offered(c, 1) == total - 3
    want = _check(c)
    assert all(3 <= len(w['src']) < 60 for w in want)


@pytest.mark.gpu
def test_gpu_merge_every_thread_suppresses():
    """640 copies of one box with distinct scores: the best suppresses every other, whichever thread
    of the workgroup and whichever of its strides the other falls to."""
    c = _inputs(1, 10, 64, seed=12, counts=[64] * 10)
    c['rois'][:, 1:] = DST
    c['boxes'][:] = c['boxes'][0, 0]
    c['scores'][:] = (np.random.default_rng(12).permutation(640) + 1).reshape(10, 64).astype(np.float32) / 1024
    want = _check(c)[0]
    assert want['src'].tolist() == [int(np.argmax(c['scores']))]


@pytest.mark.gpu
def test_gpu_merge_many_survivors():
    """Survivors far down the sorted order, between long runs of suppressed candidates and across the
    64-flag groups the greedy pass scans."""
    c = _inputs(1, 8, 64, seed=9, counts=[64] * 8, clusters=150, half=0.004)
    c['K'] = 512
    want = _check(c)[0]
    assert 80 < len(want['src']) < 400


@pytest.mark.gpu
def test_gpu_merge_frames_with_different_counts():
    counts = np.random.default_rng(10).integers(0, 9, 7 * 5)
    counts[5:10] = 0                                    # frame 1: nothing
    counts[10:15] = 8                                   # frame 2: full
    counts[15:20] = [0, 0, 1, 0, 0]                     # frame 3: one candidate
    c = _inputs(7, 5, 8, seed=10, counts=counts, clusters=25, half=0.03)
    want = _check(c)
    assert len(want[1]['src']) == 0 and want[3]['src'].tolist() == [16]
    assert len(set(len(w['src']) for w in want)) >= 4


# ---- end to end ----------------------------------------------------------------------------------

M_FACES = 8
TILE, OVERLAP, K_OUT = 64, 16, 32


@pytest.fixture(scope='module')
def e2e():
    """The seeded noise frames of tests/test_rois.py, the tile table, and the per-ROI detections
    (detect_rois) merged by the restatement; computed once."""
    from hpe.detector import BlazeFaceDetector
    from hpe.preprocess import tile_rois
    u8 = _u8((4, 96, 160, 3), seed=11)
    mc, w = fixture(RID)
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.15, max_faces=M_FACES)
    rois, per = tile_rois(4, 96, 160, TILE, OVERLAP)
    assert per == 7
    parts = det.detect_rois(u8, rois)
    packed = _pack(parts, M_FACES)
    merged = MR.merge(rois, per, packed['count'], packed['scores'], packed['boxes'], packed['keypoints'],
                      packed['poses'], (0, 0, 160, 96), det.iouThreshold, K_OUT)
    return dict(u8=u8, det=det, fixture=(mc, w), rois=rois, per=per, packed=packed, merged=merged)


def _pack(results, M):
    """[Results] per ROI image -> the arrays hpe_detect wrote for them (unused slots: a poison value)."""
    m = len(results)
    p = dict(count=np.int32([len(r.scores) for r in results]), scores=np.full((m, M), np.nan, np.float32),
             boxes=np.full((m, M, 4), 1e300), keypoints=np.full((m, M, 6, 2), 1e300),
             poses=np.full((m, M, 3), np.nan, np.float32))
    for i, r in enumerate(results):
        for k in FIELDS:
            p[k][i, :len(r.scores)] = getattr(r, k)
    return p


def _same(a, b, fields=FIELDS + ('roi', 'src')):
    for f in fields:
        _bits_equal(getattr(a, f), getattr(b, f), f)


@pytest.mark.gpu
def test_gpu_detect_tiled_equals_its_parts(e2e):
    det, merged, per = e2e['det'], e2e['merged'], e2e['per']
    got = det.detect_tiled(e2e['u8'], tile=TILE, overlap=OVERLAP, max_faces=K_OUT)
    assert len(got) == 4
    offered = [int(e2e['packed']['count'][f * per:(f + 1) * per].sum()) for f in range(4)]
    kept = [len(g.scores) for g in got]
    print('detect_tiled on the noise frames: kept %s of %s offered' % (kept, offered))
    for g, w in zip(got, merged):
        for k in FIELDS + ('src',):
            _bits_equal(getattr(g, k), w[k], k)
        _bits_equal(g.roi, (w['src'] // M_FACES).astype(np.int32), 'roi')
        assert g.refined.shape == g.scores.shape and not g.refined.any()
    # not vacuous: every frame has faces from two rows or more, and somewhere the merge removed one
    assert all(len(set(g.roi.tolist())) >= 2 for g in got)
    assert any(k < o for k, o in zip(kept, offered))
    assert all(k <= K_OUT for k in kept)
    # overlap=None is tile // 4
    for a, b in zip(det.detect_tiled(e2e['u8'], tile=TILE, max_faces=K_OUT), got):
        _same(a, b)


@pytest.mark.gpu
def test_gpu_merge_rois_method_equals_twin(e2e):
    """BlazeFaceDetector.merge_rois on postprocess()'s device dict and the device table."""
    import torch
    from hpe.preprocess import prepare_rois
    det, per = e2e['det'], e2e['per']
    r = det.postprocess(det.net.forward(prepare_rois(e2e['u8'], e2e['rois'], device=det.device)))
    out = det.merge_rois(r, torch.from_numpy(e2e['rois']).to(det.device), per, (0, 0, 160, 96), max_faces=K_OUT)
    assert set(out) == {'count', 'src', 'scores', 'boxes', 'keypoints', 'poses'}
    assert all(v.is_cuda for v in out.values()) and out['boxes'].shape == (4, K_OUT, 4)
    h = {k: v.cpu().numpy() for k, v in out.items()}
    for f, w in enumerate(e2e['merged']):
        k = len(w['src'])
        assert h['count'][f] == k
        for key in ('src', 'scores', 'poses', 'boxes', 'keypoints'):
            _bits_equal(h[key][f, :k], w[key], key)
    # max_faces=None: the detector's own
    assert det.merge_rois(r, e2e['rois'], per, (0, 0, 160, 96))['scores'].shape == (4, M_FACES)
    with pytest.raises(ValueError):
        det.merge_rois(r, e2e['rois'], per + 1, (0, 0, 160, 96))


@pytest.mark.gpu
def test_gpu_whole_look_only_is_detect_images(e2e):
    det = e2e['det']
    a = det.detect_tiled(e2e['u8'], tile=None, crop='square')
    b = det.detect_images(e2e['u8'], crop='square')
    assert len(a) == len(b) == 4 and all(len(r.scores) >= 1 for r in b)
    for ra, rb in zip(a, b):
        _bits_equal(ra.scores, rb.scores, 'scores')
        _bits_equal(ra.poses, rb.poses, 'poses')
        np.testing.assert_allclose(ra.boxes, rb.boxes, rtol=0, atol=1e-12)     # the identity remap rounds
        np.testing.assert_allclose(ra.keypoints, rb.keypoints, rtol=0, atol=1e-12)
        assert not ra.roi.any() and ra.src.tolist() == list(range(len(ra.scores)))


@pytest.mark.gpu
def test_gpu_detect_tiled_chunks_and_edges(e2e):
    det, u8 = e2e['det'], e2e['u8']
    whole = det.detect_tiled(u8, tile=TILE, overlap=OVERLAP, max_faces=K_OUT, crop='square', pad_value=(1, 2, 3))
    assert any(len(r.scores) for r in whole)
    for roi_batch in (2 * 5, 2 * 5 + 3, 1):            # 5 rows per frame: two frames per chunk; one frame per chunk
        chunked = det.detect_tiled(u8, tile=TILE, overlap=OVERLAP, max_faces=K_OUT, crop='square',
                                   pad_value=(1, 2, 3), roi_batch=roi_batch)
        assert len(chunked) == 4
        for a, b in zip(chunked, whole):
            _same(a, b)
    # a single (H, W, 3) frame, tiles only
    one = det.detect_tiled(u8[2], tile=TILE, overlap=OVERLAP, full=False)
    assert len(one) == 1
    # an empty batch
    assert det.detect_tiled(u8[:0], tile=TILE) == []
    # too many rows per frame for the merge: refused before anything runs
    with pytest.raises(ValueError):
        det.detect_tiled(u8, tile=4, overlap=0)
    with pytest.raises(ValueError):
        det.detect_tiled(u8, tile=TILE, overlap=TILE)
    with pytest.raises(ValueError):
        det.detect_tiled(u8, tile=None, full=False)
    with pytest.raises(ValueError):
        det.detect_tiled(u8.astype(np.float32), tile=TILE)


@pytest.mark.gpu
def test_gpu_detect_tiled_without_faces(e2e):
    """At a 0.9 threshold no look at the noise frames finds a face (asserted, not skipped)."""
    from hpe.detector import BlazeFaceDetector
    mc, w = e2e['fixture']
    det = BlazeFaceDetector(mc, w, scoreThreshold=0.9, max_faces=M_FACES)
    assert all(len(r.scores) == 0 for r in det.detect_rois(e2e['u8'], e2e['rois']))
    got = det.detect_tiled(e2e['u8'], tile=TILE, overlap=OVERLAP)
    assert len(got) == 4
    for g in got:
        assert g.boxes.shape == (0, 4) and g.keypoints.shape == (0, 6, 2) and g.boxes.dtype == np.float64
        assert g.scores.shape == (0,) and g.poses.shape == (0, 3) and g.poses.dtype == np.float32
        assert g.roi.shape == (0,) and g.roi.dtype == np.int32 and g.src.shape == (0,)
