"""Restatement and inputs for tests/test_detect_kernel.py (hpe_detect / hpe_gather_features,
csrc/hpe_detect.hip).

detect_frame() here is oracle.detector_ref.detect_frame with the NMS written as numpy float32 array
operations (each one rounds on its own, as oracle.detector_ref._iou does scalar by scalar), so that
896 survivors cost 896 vector steps and not 400k Python calls.  The CPU tests hold it equal to the
oracle on every case with at most 64 candidates and on seeded random frames; the GPU tests compare the
kernel with it.

A frame is a dict: cls (896,) float32 logits, loc (896, 16) float32, pose0 (16, 16, 3) and pose1
(8, 8, 3) float32.  Anchors 0..511 are the 16 x 16 x 2 front ones, 512..895 the 8 x 8 x 6 back ones.
A case is a dict: frames, t (the score threshold; the kernel gets float32(log(t / (1 - t)))), iou,
max_faces.

Scores and order.  The kernel's expf and numpy's exp may differ by an ulp, so no case may let the kept
order hang on that: order_safe() states the condition.  Logits are therefore drawn from multiples of
1/64 in [-8, 8] (adjacent sigmoids differ by 5e-6 relative at 8, the bound on both sides together is
4.8e-7), or saturate: at a logit >= 20, exp(-x) <= 2.1e-9 < 2^-25, so 1 + exp(-x) rounds to 1 and the
score is exactly 1.0f whoever computes exp; at a logit <= -100, exp(-x) >= 2.7e43 is above the float32
range, so it is +inf and the score exactly 0.0f.  No logit lies in (-100, -80): there the score is a
float32 denormal and its value would depend on the device's denormal handling, which is not what these
tests are about.  Nor in (8, 20), where the sigmoid is within the bound of 1.0f.
"""
import numpy as np

from oracle import detector_ref as D

F4, F8 = np.float32, np.float64
N0, N = 512, 896
SCORE_BOUND = 2.0 ** -22      # 1 ulp of expf (2^-23) + one rounding each for the add and the divide (2 * 2^-24)
ANCHORS = D.anchors()


def logit_threshold(t):
    """float32 of the detector's log(t / (1 - t)); t = 0 gives -inf."""
    with np.errstate(divide='ignore'):
        return F4(D.score_logit_threshold(t))


def sigmoid64(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, F8)))


def sigmoid32(x):
    """The oracle's score expression (filterDetections), float32 throughout."""
    with np.errstate(over='ignore'):
        return (F4(1.0) / (F4(1.0) + np.exp(-np.asarray(x, F4)))).astype(F4)


def decode(loc, idx):
    """float64 boxes (k, 4) [x1, y1, x2, y2] and keypoints (k, 6, 2) of anchors idx, the oracle's
    extractDetections arithmetic on arrays."""
    l = np.asarray(loc, F4)[idx].astype(F8)
    ax, ay = ANCHORS[idx, 0], ANCHORS[idx, 1]
    with np.errstate(all='ignore'):
        cx = (l[:, 0] + ax * 128.0) / 128.0
        cy = (l[:, 1] + ay * 128.0) / 128.0
        w = l[:, 2] / 128.0
        h = l[:, 3] / 128.0
        boxes = np.stack([cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5], 1)
        kps = np.stack([(l[:, 4::2] + ax[:, None] * 128.0) / 128.0, (l[:, 5::2] + ay[:, None] * 128.0) / 128.0], 2)
    return boxes, kps


def iou_parts(bi, bj):
    """fp32 boxes (..., 4) against (..., 4), corner order agnostic, every operation a float32 numpy
    call: (area_i + area_j, inter height, inter width, inter, both areas positive)."""
    bi, bj = np.asarray(bi, F4), np.asarray(bj, F4)
    with np.errstate(all='ignore'):
        ymin_i, xmin_i = np.minimum(bi[..., 0], bi[..., 2]), np.minimum(bi[..., 1], bi[..., 3])
        ymax_i, xmax_i = np.maximum(bi[..., 0], bi[..., 2]), np.maximum(bi[..., 1], bi[..., 3])
        ymin_j, xmin_j = np.minimum(bj[..., 0], bj[..., 2]), np.minimum(bj[..., 1], bj[..., 3])
        ymax_j, xmax_j = np.maximum(bj[..., 0], bj[..., 2]), np.maximum(bj[..., 1], bj[..., 3])
        area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i)
        area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j)
        ih = np.maximum(np.minimum(ymax_i, ymax_j) - np.maximum(ymin_i, ymin_j), F4(0))
        iw = np.maximum(np.minimum(xmax_i, xmax_j) - np.maximum(xmin_i, xmin_j), F4(0))
        inter = ih * iw
        s = area_i + area_j
    assert s.dtype == F4 and inter.dtype == F4
    return s, ih, iw, inter, (area_i > 0) & (area_j > 0)


def iou(bi, bj):
    """tf NMS IoU in float32, inter rounded before it is subtracted (oracle.detector_ref._iou)."""
    s, _, _, inter, ok = iou_parts(bi, bj)
    with np.errstate(all='ignore'):
        v = inter / (s - inter)
    return np.where(ok, v, F4(0)).astype(F4)


def iou_contracted(bi, bj):
    """The same with the denominator as one fused multiply-add would give it:
    fp32(fp64(s) - fp64(h) * fp64(w)), the product unrounded."""
    s, ih, iw, inter, ok = iou_parts(bi, bj)
    with np.errstate(all='ignore'):
        den = (s.astype(F8) - ih.astype(F8) * iw.astype(F8)).astype(F4)
        v = inter / den
    return np.where(ok, v, F4(0)).astype(F4)


def nms(boxes32, scores, idx, max_faces, iou_threshold):
    """Greedy by score descending, ties to the lower index; positions into the inputs, kept order."""
    order = np.lexsort((idx, -scores.astype(F8)))
    b = boxes32[order]
    alive = np.ones(len(order), bool)
    thr = F4(iou_threshold)
    sel = []
    for p in range(len(order)):
        if len(sel) >= max_faces:
            break
        if not alive[p]:
            continue
        sel.append(p)
        if p + 1 < len(order):
            alive[p + 1:] &= ~(iou(b[p], b[p + 1:]) > thr)
    return order[np.asarray(sel, np.int64)]


def detect_frame(fr, t=0.4, iou_threshold=0.3, max_faces=D.MAX_FACE_NUM):
    """oracle.detector_ref.detect_frame on a frame dict, same keys in the result."""
    cls = np.asarray(fr['cls'], F4)
    good = np.where(cls > logit_threshold(t))[0]
    scores = sigmoid32(cls[good])
    boxes, kps = decode(fr['loc'], good)
    with np.errstate(over='ignore', invalid='ignore'):
        b32 = boxes.astype(F4)
    sel = nms(b32, scores, good, max_faces, iou_threshold)
    det = good[sel]
    front = det < N0
    cell = np.where(front, det // 2, (det - N0) // 6)
    poses = np.where(front[:, None], fr['pose0'].reshape(256, 3)[np.where(front, cell, 0)],
                     fr['pose1'].reshape(64, 3)[np.where(front, 0, cell)]).astype(F4).reshape(-1, 3)
    return dict(det_index=det, scores=scores[sel], boxes=boxes[sel], keypoints=kps[sel], poses=poses)


def oracle_frame(fr, t=0.4, iou_threshold=0.3, max_faces=D.MAX_FACE_NUM):
    with np.errstate(over='ignore', divide='ignore'):
        return D.detect_frame(fr['cls'][:N0], fr['cls'][N0:], fr['loc'][:N0], fr['loc'][N0:], fr['pose0'],
                              fr['pose1'], score_threshold=t, iou_threshold=iou_threshold, max_faces=max_faces)


def candidates(fr, t):
    return np.where(np.asarray(fr['cls'], F4) > logit_threshold(t))[0]


def order_safe(fr, t):
    """The kept order cannot depend on whose exp is used: every candidate logit is one of the module
    docstring's three kinds, and distinct unsaturated ones differ by more than twice the score bound."""
    x = np.unique(fr['cls'][candidates(fr, t)].astype(F8))
    hi, lo = x >= 20, x <= -100
    if not (hi | lo | ((x >= -80) & (x <= 8))).all():
        return False
    s = np.unique(np.where(hi, 1.0, np.where(lo, 0.0, sigmoid64(np.clip(x, -100, 20)))))
    return bool((np.diff(s) > 2 * SCORE_BOUND * s[1:]).all())


# ---- inputs ---------------------------------------------------------------------------------------

def grid_logits(rng, size, lo, hi):
    """Multiples of 1/64 in [lo / 64, hi / 64]."""
    return (rng.integers(lo, hi + 1, size) / 64.0).astype(F4)


def blank(seed, fill=-10.0):
    """Nothing above any threshold used here (but -inf's); random boxes 8..40 pixels wide around their
    anchors, random keypoints and poses."""
    rng = np.random.default_rng(seed)
    loc = rng.normal(0, 4, (N, 16)).astype(F4)
    loc[:, 2:4] = rng.uniform(8, 40, (N, 2))
    return dict(cls=np.full(N, fill, F4), loc=loc, pose0=rng.normal(0, 20, (16, 16, 3)).astype(F4),
                pose1=rng.normal(0, 20, (8, 8, 3)).astype(F4))


def random_frame(seed, k):
    """Exactly k candidates at t = 0.4 (threshold logit -0.405...): theirs are multiples of 1/64 in
    [-25/64, 8], the others' in [-8, -26/64]; many ties."""
    rng = np.random.default_rng(seed)
    fr = blank(seed)
    fr['cls'] = grid_logits(rng, N, -512, -26)
    on = rng.permutation(N)[:k]
    fr['cls'][on] = grid_logits(rng, k, -25, 512)
    return fr


def place(fr, d, x, y, w, h):
    """Anchor d's box: centre (x, y) and size (w, h) in pixels of the 128 x 128 input (exact when the
    numbers are small dyadic rationals: anchor centres are multiples of 4 pixels)."""
    fr['loc'][d, 0] = x - ANCHORS[d, 0] * 128.0
    fr['loc'][d, 1] = y - ANCHORS[d, 1] * 128.0
    fr['loc'][d, 2] = w
    fr['loc'][d, 3] = h


def all_anchors_frame(seed=21):
    """Every anchor above the threshold with a box of its own, disjoint from every other: rows of
    boxes at most 1.4 pixels high (jitter included), the front anchors of a cell 2 pixels below its
    centre (y = 6 mod 8), the back ones level with theirs (y = 0 mod 8), 2 pixels apart along x."""
    rng = np.random.default_rng(seed)
    fr = blank(seed)
    fr['cls'] = grid_logits(rng, N, 0, 512)
    fr['loc'][:] = rng.normal(0, 4, (N, 16))
    dx = np.where(np.arange(N) < N0, (np.arange(N) % 2) * 4.0 - 2.0, ((np.arange(N) - N0) % 6) * 2.0 - 5.0)
    dy = np.where(np.arange(N) < N0, 2.0, 0.0)
    fr['loc'][:, 0] = dx + rng.uniform(-0.2, 0.2, N)
    fr['loc'][:, 1] = dy + rng.uniform(-0.2, 0.2, N)
    fr['loc'][:, 2:4] = rng.uniform(0.5, 1.0, (N, 2))
    return fr


def same_box_frame(seed=22):
    """896 copies of one box (bit-identical after the decode), distinct logits."""
    fr = blank(seed)
    for d in range(N):
        place(fr, d, 64.0, 60.0, 24.0, 20.0)
    fr['cls'] = (np.random.default_rng(seed).permutation(N) / 128.0).astype(F4)     # 7.1e-6 apart at 7
    return fr


def threshold_frame(t, seed=23):
    """Logits at the float32 threshold (dropped), one float32 above (kept) and below (dropped), NaN and
    -inf (dropped), +inf (kept, score 1), +-0 (dropped when the threshold is 0), on every 16th anchor
    (the others -inf); every box disjoint, so what is above the threshold is kept."""
    thr = logit_threshold(t)
    fr = all_anchors_frame(seed)
    vals = [thr, np.nextafter(thr, F4(np.inf)), np.nextafter(thr, F4(-np.inf)), F4(np.nan), F4(np.inf), F4(-np.inf),
            F4(0.0), F4(-0.0)]
    fr['cls'][:] = -np.inf
    fr['cls'][::16] = [vals[j % 8] for j in range(N // 16)]      # 7 of each, 32 front and 24 back anchors
    if thr < 0:                           # where 0 is above the threshold it is a plain candidate: not here
        fr['cls'][fr['cls'] == 0] = F4(-np.inf)
    return fr


def saturated_high_frame(seed=24, k=50):
    """k distinct logits in [20, 80] on overlapping boxes: every score 1.0f, the order by index."""
    rng = np.random.default_rng(seed)
    fr = blank(seed)
    on = rng.permutation(N)[:k]
    fr['cls'][on] = rng.permutation(4096)[:k].astype(F4) * F4(60.0 / 4096) + F4(20.0)
    return fr


def saturated_low_frame(seed=25, k=N):
    """k distinct logits in [-200, -100] (the rest -inf) for a -inf threshold: every score 0.0f."""
    rng = np.random.default_rng(seed)
    fr = blank(seed, fill=-np.inf)
    on = rng.permutation(N)[:k]
    fr['cls'][on] = -(rng.permutation(4096)[:k].astype(F4) * F4(100.0 / 4096) + F4(100.0))
    return fr


def flipped_frame(seed=26, k=48):
    """Negative widths and / or heights (the corners come out swapped)."""
    fr = random_frame(seed, k)
    on = candidates(fr, 0.4)
    fr['loc'][on[0::4], 2] *= -1
    fr['loc'][on[1::4], 3] *= -1
    fr['loc'][on[2::4], 2:4] *= -1
    return fr


def zero_area_frame(seed=27):
    """Identical zero-width boxes, identical zero-height ones and a 0 x 0 one inside a large box that
    outscores some and not others, and inside another that the large one suppresses."""
    fr = blank(seed)
    logit = iter(np.arange(40, 0, -1) / 8.0)
    place(fr, 3, 64, 64, 40, 40)
    fr['cls'][3] = 3.0
    place(fr, 600, 66, 62, 36, 36)          # IoU with anchor 3's box 0.81: suppressed
    fr['cls'][600] = 2.5
    for d in (10, 11, 700, 12):              # zero width, the same box four times
        place(fr, d, 64, 64, 0, 16)
        fr['cls'][d] = next(logit)
    for d in (20, 701, 21):                  # zero height
        place(fr, d, 60, 70, 16, 0)
        fr['cls'][d] = next(logit)
    place(fr, 30, 64, 64, 0, 0)
    fr['cls'][30] = 1.0
    return fr


def contained_frame(seed=28):
    """One box inside another: IoU = the area ratio.  36 / 64 (suppressed at 0.3), 16 / 64 (kept),
    and the same two with the inner box the better one."""
    fr = blank(seed)
    place(fr, 0, 32, 32, 32, 32)
    place(fr, 1, 30, 34, 24, 24)
    place(fr, 520, 36, 28, 16, 16)
    place(fr, 300, 96, 96, 16, 16)
    place(fr, 301, 96, 96, 32, 32)
    place(fr, 880, 96, 96, 24, 24)
    fr['cls'][[0, 1, 520, 300, 301, 880]] = [4.0, 3.0, 2.0, 3.5, 1.5, 2.5]
    return fr


def nonfinite_frame(seed=29, k=60):
    fr = random_frame(seed, k)
    on = candidates(fr, 0.4)
    fr['loc'][on[0], 0] = np.nan
    fr['loc'][on[1], 3] = np.nan
    fr['loc'][on[2], 2] = np.inf
    fr['loc'][on[3], 1] = -np.inf
    fr['loc'][on[4], :4] = np.nan
    fr['loc'][on[5], 7] = np.nan             # a keypoint only
    return fr


def case(frames, t=0.4, iou=0.3, max_faces=D.MAX_FACE_NUM):
    return dict(frames=frames if isinstance(frames, list) else [frames], t=t, iou=iou, max_faces=max_faces)


COUNTS = (0, 1, 255, 256, 257, 896)


def cases():
    """Every hpe_detect case of tests/test_detect_kernel.py whose result is compared with the
    restatement, by name (the IoU pairs come from iou_pairs / exact_third_frame)."""
    c = {}
    for t in (0.4, 0.5, 1e-30):
        c['threshold_%g' % t] = case(threshold_frame(t), t=t, max_faces=N)
    c['threshold_minus_inf'] = case(saturated_low_frame(seed=30, k=40), t=0.0)
    c['threshold_minus_inf_mixed'] = case(threshold_frame(0.0), t=0.0, max_faces=N)
    c['saturated_high'] = case(saturated_high_frame())
    c['saturated_low_896'] = case(saturated_low_frame(), t=0.0)
    c['saturated_low_40'] = case(saturated_low_frame(seed=31, k=40), t=0.0)
    for m in (1, 7, 100, N, 1000):
        c['all_anchors_max_%d' % m] = case(all_anchors_frame(), max_faces=m)
    c['flipped'] = case(flipped_frame())
    c['zero_area'] = case(zero_area_frame())
    c['contained'] = case(contained_frame())
    c['same_box_896'] = case(same_box_frame())
    c['disjoint'] = case(threshold_frame(0.4, seed=32), max_faces=7)
    c['counts'] = case([random_frame(40 + i, k) for i, k in enumerate(COUNTS)], max_faces=120)
    c['six_frames'] = case([random_frame(50 + i, k) for i, k in enumerate((300, 17, 0, 640, 64, 130))])
    return c


def iou_pairs(seed=7, n=1 << 16, want=8):
    """Seeded search over fp32 loc pairs of anchors 0 and 1 (one cell, so the boxes overlap), decoded
    as the kernel decodes them: pairs whose IoU with the rounded inter differs from the contracted
    form.  Returns (higher, lower): lists of (loc_a (4,), loc_b (4,), reference IoU float32), `want`
    of each, the contracted value one above / one below the reference."""
    rng = np.random.default_rng(seed)
    loc = np.zeros((2 * n, 16), F4)
    loc[:, :2] = rng.uniform(-6, 6, (2 * n, 2))
    loc[:, 2:4] = rng.uniform(8, 40, (2 * n, 2))
    d = np.tile(np.arange(2), n)
    l = loc.astype(F8)
    cx, cy = (l[:, 0] + 4.0) / 128.0, (l[:, 1] + 4.0) / 128.0     # anchors 0 and 1: centre (4, 4) pixels
    w, h = l[:, 2] / 128.0, l[:, 3] / 128.0
    b = np.stack([cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5], 1).astype(F4)
    assert (d[0::2] == 0).all()
    ref, con = iou(b[0::2], b[1::2]), iou_contracted(b[0::2], b[1::2])
    out = []
    for pick in (con > ref, con < ref):
        at = np.where(pick & (ref > 0.05) & (ref < 0.95))[0][:want]
        out.append([(loc[2 * i, :4].copy(), loc[2 * i + 1, :4].copy(), ref[i]) for i in at])
    return out


def pair_frame(loc_a, loc_b, seed=33):
    """Anchors 0 (the better score) and 1 with the pair's boxes; nothing else above the threshold."""
    fr = blank(seed)
    fr['loc'][0, :4] = loc_a
    fr['loc'][1, :4] = loc_b
    fr['cls'][0], fr['cls'][1] = 2.0, 1.0
    return fr


def exact_third_frames():
    """Pairs whose IoU is float32(1/3) with every intermediate exact (sizes and offsets powers of two):
    tests/test_detector.py's [0, 0, 1, 1] / [0.5, 0, 1.5, 1] in three places and sizes, once flipped."""
    out = []
    for k, (d0, d1, x, y, s, sign) in enumerate([(0, 1, 16, 16, 16, 1), (100, 612, 64, 32, 32, 1), (800, 30, 48, 80, 8, -1)]):
        fr = blank(34 + k)
        place(fr, d0, x, y, s, s)
        place(fr, d1, x + s / 2, y, sign * s, s)
        fr['cls'][d0], fr['cls'][d1] = 2.0, 1.0
        out.append((fr, d0, d1))
    return out
