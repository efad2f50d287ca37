"""Restatement of the face tracker (hpe_track / hpe_track_reset, csrc/hpe_track.hip) that the kernel
must equal bit for bit.

Plain Python over numpy scalars, one rounded operation per expression: float64 for the smoothing
(state = alpha * m + (1.0 - alpha) * state, hpe.detector.EMAFilter.update), float32 for the IoU on the
float32 casts of the boxes (tests/detect_ref.py's iou, the one restatement of oracle.detector_ref._iou
the tests use: a non-positive or NaN area gives 0, as csrc/hpe_boxes.h has it).  The state arrays are
updated in place, as the kernel updates them.
"""
import numpy as np

from detect_ref import iou

STATE_D = 23     # HPE_TRACK_STATE_D
NV = 19          # smoothed values per track: box 4, keypoints 12, pose 3
MAX_TRACKS = 64  # HPE_TRACK_MAX_TRACKS
F4, F8 = np.float32, np.float64


def new_state(n_streams, max_tracks):
    """What hpe_track_reset writes: next_id 0, ids -1, misses 0, doubles 0.0."""
    K = int(max_tracks)
    si = np.zeros((n_streams, 1 + 2 * K), np.int32)
    si[:, 1:1 + K] = -1
    return si, np.zeros((n_streams, K, STATE_D), F8)


def track(n_streams, n_frames, count, boxes, keypoints, poses, alpha, match_iou, max_missed, state_i, state_d,
          track_out, boxes_out, keypoints_out, poses_out):
    """The arguments of hpe_track as numpy arrays (max_faces and max_tracks are their shapes); state and
    outputs are written in place, output slots at or past a frame's clamped count are left alone."""
    S, T = int(n_streams), int(n_frames)
    M = boxes.shape[1]
    K = state_d.shape[1]
    alpha = F8(alpha)
    om = F8(1.0) - alpha
    thr = F4(match_iou)
    for s in range(S):
        si, sd = state_i[s], state_d[s]
        for t in range(T):
            g = s * T + t
            c = min(max(int(count[g]), 0), M)
            matched = [False] * K
            for j in range(c):
                m = np.concatenate([boxes[g, j], keypoints[g, j].reshape(12), poses[g, j].astype(F8)])
                w, hit = -1, False
                if np.isfinite(boxes[g, j]).all():
                    with np.errstate(over='ignore'):
                        b32 = boxes[g, j].astype(F4)
                        best = None
                        for q in range(K):
                            if si[1 + q] < 0 or matched[q]:
                                continue
                            u = iou(b32, sd[q, NV:].astype(F4))
                            if u > thr and (best is None or u > best):   # NaN never qualifies
                                best, w, hit = u, q, True
                    if not hit:
                        free = [q for q in range(K) if si[1 + q] < 0]
                        if free:
                            w = free[0]
                            si[1 + w] = si[0]
                            si[0] = np.int32((int(si[0]) + 1) & 0x7fffffff)
                            sd[w, :NV] = m
                if w < 0:
                    track_out[g, j] = -1
                    boxes_out[g, j] = boxes[g, j]
                    keypoints_out[g, j] = keypoints[g, j]
                    poses_out[g, j] = poses[g, j]
                    continue
                if hit:
                    with np.errstate(all='ignore'):
                        for e in range(NV):
                            sd[w, e] = F8(alpha * m[e]) + F8(om * sd[w, e])
                matched[w] = True
                si[1 + K + w] = 0
                sd[w, NV:] = boxes[g, j]
                track_out[g, j] = si[1 + w]
                boxes_out[g, j] = sd[w, :4]
                keypoints_out[g, j] = sd[w, 4:16].reshape(6, 2)
                with np.errstate(over='ignore'):
                    poses_out[g, j] = sd[w, 16:NV].astype(F4)
            for q in range(K):
                if si[1 + q] >= 0 and not matched[q]:
                    si[1 + K + q] += 1
                    if si[1 + K + q] > max_missed:
                        si[1 + q] = -1


def run(n_streams, count, boxes, keypoints, poses, alpha, match_iou, max_missed, max_tracks, state=None):
    """Convenience: fresh (or given, copied) state, sentinel-filled outputs -> (track, boxes, keypoints,
    poses, state_i, state_d)."""
    n = len(count)
    M = boxes.shape[1]
    si, sd = new_state(n_streams, max_tracks) if state is None else (state[0].copy(), state[1].copy())
    out = outputs(n, M)
    track(n_streams, n // n_streams if n_streams else 0, count, boxes, keypoints, poses, alpha, match_iou,
          max_missed, si, sd, *out)
    return out + (si, sd)


SENT_I = np.int32(-777)
SENT_D = F8(-1234.5)
SENT_F = F4(-4321.5)


def outputs(n, M):
    """Output buffers pre-filled with the sentinels."""
    return (np.full((n, M), SENT_I, np.int32), np.full((n, M, 4), SENT_D, F8), np.full((n, M, 6, 2), SENT_D, F8),
            np.full((n, M, 3), SENT_F, F4))
