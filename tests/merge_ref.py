"""Restatement of tiled detection's host table (hpe.preprocess.tile_rois) and of its merge kernel
(hpe_merge_rois, csrc/hpe_merge.hip) that both must equal exactly.

The table is the issue's integer arithmetic written out again.  The merge is numpy float64, one
rounded operation per numpy call, then oracle.detector_ref.non_max_suppression on the float32 casts of
the remapped boxes: the candidates are handed over in r * M + j order, so its tie-break (the lower
position) is the kernel's.
"""
import numpy as np

import roi_ref as R
from oracle.detector_ref import non_max_suppression

MAX_CAND = 4096
F8 = np.float64


def crop_rect(h, w, crop):
    if crop is None:
        return 0, 0, w, h
    if crop == 'square':
        s = min(h, w)
        return (w - s) // 2, (h - s) // 2, s, s
    return tuple(int(c) for c in crop)


def offsets(L, tile, overlap):
    if L <= tile:
        return [-((tile - L) // 2)]
    step = tile - overlap
    n = (L - tile + step - 1) // step + 1
    return [(i * (L - tile)) // (n - 1) for i in range(n)]


def tile_rois(n_frames, h, w, tile, overlap, crop=None, full=True):
    sx, sy, sw, sh = crop_rect(h, w, crop)
    rows = [(sx, sy, sw, sh)] if full else []
    if tile is not None:
        for oy in offsets(sh, tile, overlap):
            for ox in offsets(sw, tile, overlap):
                rows.append((sx + ox, sy + oy, tile, tile))
    rois = np.array([(f,) + r for f in range(n_frames) for r in rows], np.int32).reshape(-1, 5)
    return rois, len(rows)


def remap(xy, roi, dst):
    """(..., 2) float64 points normalised to the row (f, rx, ry, rw, rh) -> normalised to dst =
    (x0, y0, w, h): X = ((rx + x * rw) - x0) / w, likewise Y, each operation rounded on its own."""
    xy = np.asarray(xy, F8)
    _, rx, ry, rw, rh = (F8(int(v)) for v in roi)
    dx0, dy0, dw, dh = (F8(int(v)) for v in dst)
    with np.errstate(all='ignore'):
        X = np.divide(np.subtract(np.add(rx, np.multiply(xy[..., 0], rw)), dx0), dw)
        Y = np.divide(np.subtract(np.add(ry, np.multiply(xy[..., 1], rh)), dy0), dh)
    return np.stack([X, Y], -1)


def merge(rois, rows_per_frame, count, scores, boxes, keypoints, poses, dst, iou_threshold, max_faces_out):
    """rois (n * R, 5); count (n * R,), scores (n * R, M) float32, boxes (n * R, M, 4) float64, keypoints
    (n * R, M, 6, 2) float64, poses (n * R, M, 3) float32 -> one dict per frame of src int32, scores,
    boxes, keypoints, poses in selection order."""
    rois = np.asarray(rois)
    Rr = int(rows_per_frame)
    n = len(rois) // Rr
    M = scores.shape[1]
    out = []
    for f in range(n):
        src, bx = [], []
        for r in range(Rr):
            row = f * Rr + r
            if not (R.valid(rois[row], n) and int(rois[row, 0]) == f):
                continue
            for j in range(min(max(int(count[row]), 0), M)):
                b = remap(boxes[row, j].reshape(2, 2), rois[row], dst).reshape(4)
                if np.isfinite(b).all() and not np.isnan(scores[row, j]):
                    src.append(r * M + j)
                    bx.append(b)
        src = np.asarray(src, np.int64)
        if len(src):
            rr, jj = f * Rr + src // M, src % M
            with np.errstate(over='ignore'):
                b32 = np.asarray(bx, F8).astype(np.float32)
            sel = non_max_suppression(b32, scores[rr, jj], max_faces_out, iou_threshold)
            src = src[sel]
        rr, jj = f * Rr + src // M, src % M
        out.append(dict(
            src=src.astype(np.int32),
            scores=scores[rr, jj].copy(),
            poses=poses[rr, jj].reshape(-1, 3).copy(),
            boxes=np.array([remap(boxes[a, b].reshape(2, 2), rois[a], dst).reshape(4) for a, b in zip(rr, jj)],
                           F8).reshape(-1, 4),
            keypoints=np.array([remap(keypoints[a, b], rois[a], dst) for a, b in zip(rr, jj)],
                               F8).reshape(-1, 6, 2)))
    return out
