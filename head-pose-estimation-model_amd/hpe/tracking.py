"""Faces tracked across video frames and their box, keypoints and pose smoothed on the device
(csrc/hpe_track.hip, C ABI ``hpe_track`` / ``hpe_track_reset``; the rules are written out in
include/hpe.h).

The reference's webcam loop smooths every face with 19 ``EMAFilter``s that it indexes by the face's
position in the frame's result list (BlazePoser/blazeFaceDetectorH5.py:383-425), which holds while
exactly one face is in view.  ``PoseTracker`` puts an association step in front of the same arithmetic
(IoU against each track's last raw box, greedy in the frame's NMS order), keeps the state on the device
from call to call, so a long video streams through in chunks, and never reads the host.
"""
import torch

from . import _lib
from ._lib import ptr as _ptr
from .preprocess import _launch

MAX_TRACKS = 64   # HPE_TRACK_MAX_TRACKS
STATE_D = 23      # HPE_TRACK_STATE_D: 19 smoothed values and the last matched raw box per track


class PoseTracker:
    """Tracks the faces of ``streams`` independent videos.

    alpha: the EMA weight of a new measurement; 0.15 is the reference's (blazeFaceDetectorH5.py:378).
    match_iou: a detection continues the track whose last raw box it overlaps most, if that IoU is above
    match_iou (negative: any live track matches, the reference's position-only filter for one face).
    max_missed: a track not matched for more than this many consecutive frames is dropped.
    max_tracks: track slots per stream (1 .. 64); a detection that finds neither a track nor a free slot
    comes back untracked (id -1, values as detected).
    The defaults of match_iou, max_missed and max_tracks are unmeasured: the reference has no
    counterpart, and no data set was run to choose them.
    """

    def __init__(self, alpha=0.15, match_iou=0.3, max_missed=5, max_tracks=8, streams=1, device=None):
        self.alpha = float(alpha)
        self.match_iou = float(match_iou)
        self.max_missed = int(max_missed)
        self.max_tracks = int(max_tracks)
        self.streams = int(streams)
        if self.streams < 1:
            raise ValueError('PoseTracker: streams must be positive, got %r' % (streams,))
        if not 1 <= self.max_tracks <= MAX_TRACKS:
            raise ValueError('PoseTracker: max_tracks %r outside 1 .. %d' % (max_tracks, MAX_TRACKS))
        self.device = torch.device('cuda' if device is None else device)
        S, K = self.streams, self.max_tracks
        self.state_i = torch.empty((S, 1 + 2 * K), dtype=torch.int32, device=self.device)
        self.state_d = torch.empty((S, K, STATE_D), dtype=torch.float64, device=self.device)
        self.reset()

    def reset(self):
        """Forget every track: the next frame starts each video anew, ids from 0."""
        _launch('hpe_track_reset', self.device, self.streams, self.max_tracks, _ptr(self.state_i),
                _ptr(self.state_d))

    def update(self, r):
        """r: the device dict of BlazeFaceDetector.postprocess or merge_rois for streams * T images,
        stream-major (image s * T + t is frame t of video s), the frames that follow the previous call's.
        Returns a device dict: ``count`` and ``scores`` passed through, ``track`` (n, M) int32 the face's
        id (-1: untracked) and the smoothed ``boxes``, ``keypoints``, ``poses``; slots past count are not
        written.  No host read."""
        n, M = r['boxes'].shape[0], r['boxes'].shape[1]
        if n % self.streams:
            raise ValueError('PoseTracker.update: %d images are not a whole number of frames for %d streams'
                             % (n, self.streams))
        dev = self.device
        count = r['count'].to(dev, torch.int32).contiguous()
        boxes = r['boxes'].to(dev, torch.float64).contiguous()
        kps = r['keypoints'].to(dev, torch.float64).contiguous()
        poses = r['poses'].to(dev, torch.float32).contiguous()
        out = dict(count=r['count'], scores=r['scores'],
                   track=torch.empty((n, M), dtype=torch.int32, device=dev),
                   boxes=torch.empty_like(boxes), keypoints=torch.empty_like(kps), poses=torch.empty_like(poses))
        _launch('hpe_track', dev, self.streams, n // self.streams, M, _ptr(count), _ptr(boxes), _ptr(kps),
                _ptr(poses), self.alpha, self.match_iou, self.max_missed, self.max_tracks, _ptr(self.state_i),
                _ptr(self.state_d), _ptr(out['track']), _ptr(out['boxes']), _ptr(out['keypoints']),
                _ptr(out['poses']))
        return out

    def state(self):
        """Host copies (state_i (S, 1 + 2K) int32, state_d (S, K, 23) float64), laid out as include/hpe.h
        describes."""
        return self.state_i.cpu().numpy(), self.state_d.cpu().numpy()
