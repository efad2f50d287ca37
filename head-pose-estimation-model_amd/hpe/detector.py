"""Batched face detection + head pose: the unified BlazeFace graph (hpe.blazeface) followed by the
detector post-processing kernel (csrc/hpe_detect.hip, C ABI ``hpe_detect``).

Mirrors ``blazeFaceDetector`` of BlazePoser/blazeFaceDetectorH5.py:80-364: ``detectFaces(frame)`` for
one frame and ``detect_batch(frames)`` for a batch, returning ``Results(boxes, keypoints, scores,
poses)`` per frame (:359-364).  uint8 input is a raw camera frame, as the reference's ``detectFaces``
takes it (BGR): ``detect_images`` prepares it on the device (``prepareInputForInference``, :247-269:
RGB, /255, bicubic resize to 128x128, (x - 0.5) / 0.5 — hpe.preprocess, csrc/hpe_preproc.hip).  Float
input is the already prepared model input.  ``detect_rois`` runs the detector on regions of interest of
the frames (hpe_preprocess_rois) and ``detect_refine`` looks a second time at an enlarged square around
every face of a first pass (hpe_face_rois); ``detect_tiled`` looks at every frame as a whole and in
overlapping tiles and merges the looks per frame on the device (hpe.preprocess.tile_rois,
csrc/hpe_merge.hip, C ABI ``hpe_merge_rois``); none of the three is in the reference.  Wherever raw
frames go, decoded NV12 video goes too, wrapped in hpe.preprocess.NV12Frames.  ``EMAFilter``
is the webcam loop's pose smoothing (:16-35), one scalar at a time on the host; ``detect_video`` does
for a batch of video frames what that loop does per frame (:383-425: the 19 filters of a face's box,
keypoints and angles) on the device, with the faces associated across frames first
(hpe.tracking.PoseTracker, csrc/hpe_track.hip, C ABI ``hpe_track``).  ``draw`` is the loop's last stage,
``drawDetections`` (:175-219: box, keypoints and pose axes, without the text), on the device and in place
for device frames (hpe.draw, csrc/hpe_draw.hip, C ABI ``hpe_pose_prims`` / ``hpe_draw`` / ``hpe_draw_nv12``).
Webcam capture is out of scope.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr
from .blazeface import BlazeFace
from .draw import DrawStyle, draw_prims, pack_results, pose_prims
from .preprocess import (NV12Frames, _checked_frames, _device_frames, _launch, crop_rect, frame_dims, prepare_input,
                         prepare_rois, roi_table, tile_rois)

KEY_POINT_SIZE = 6      # blazeFaceDetectorH5.py:8
MAX_FACE_NUM = 100      # blazeFaceDetectorH5.py:9
MERGE_MAX_CAND = 4096   # HPE_MERGE_MAX_CAND: rows per frame x max_faces that hpe_merge_rois takes


class Results:
    def __init__(self, boxes, keypoints, scores, poses):
        self.boxes = boxes
        self.keypoints = keypoints
        self.scores = scores
        self.poses = poses
        self.refined = np.zeros(len(scores), bool)   # detect_refine: the second pass replaced this face
        # detect_tiled: the table row within the frame each face came from (0: the whole look when
        # full) and its candidate index row * max_faces + slot among the frame's per-ROI detections
        self.roi = np.zeros(len(scores), np.int32)
        self.src = np.zeros(len(scores), np.int32)
        self.track = np.full(len(scores), -1, np.int32)   # detect_video: the face's id across frames


class EMAFilter:
    """Exponential moving average of a measurement (blazeFaceDetectorH5.py:16-35); the first
    measurement passes through."""

    def __init__(self, alpha, initial_value=0.0):
        assert 0.0 < alpha <= 1.0, 'alpha must be in (0,1]'
        self.alpha = alpha
        self.state = initial_value
        self.initialized = False

    def update(self, measurement):
        if not self.initialized:
            self.state = measurement
            self.initialized = True
        else:
            self.state = self.alpha * measurement + (1.0 - self.alpha) * self.state
        return self.state


def is_uint8(frames):
    """Raw camera frames (uint8 BGR, or NV12Frames) as opposed to the prepared float model input."""
    if isinstance(frames, NV12Frames):
        return True
    if torch.is_tensor(frames):
        return frames.dtype == torch.uint8
    return isinstance(frames, np.ndarray) and frames.dtype == np.uint8


def remap_roi(xy, rx, ry, side, src):
    """(..., 2) float64 points normalised to the square ROI (rx, ry, side) -> normalised to the source
    rectangle src = (x0, y0, w, h): X = (rx + x * side - x0) / w, likewise in y."""
    xy = np.asarray(xy, np.float64)
    return np.stack([(rx + xy[..., 0] * side - src[0]) / src[2], (ry + xy[..., 1] * side - src[1]) / src[3]], -1)


def _device_input(frames, device):
    """Prepared float frames, numpy array or tensor -> the contiguous float32 tensor on ``device``."""
    x = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames, np.float32))
    return x.to(device, torch.float32).contiguous()


def _host_results(r, copy=False):
    """r: postprocess()'s dict -> [Results] * n on the host; copy: for a caller that writes into them."""
    h = {k: v.cpu().numpy() for k, v in r.items()}
    res = []
    for i, c in enumerate(int(c) for c in h['count']):
        f = [h['boxes'][i, :c], h['keypoints'][i, :c], h['scores'][i, :c],
             h['poses'][i, :c] if c else np.zeros((0, 3), np.float32)]
        res.append(Results(*([a.copy() for a in f] if copy else f)))
    return res


class BlazeFaceDetector:
    def __init__(self, model_config, weights, scoreThreshold=0.4, iouThreshold=0.3, device=None,
                 max_faces=MAX_FACE_NUM):
        self.scoreThreshold = scoreThreshold
        self.iouThreshold = iouThreshold
        self.sigmoidScoreThreshold = math.log(scoreThreshold / (1 - scoreThreshold))
        self.max_faces = int(max_faces)
        self.net = BlazeFace(model_config, weights, device=device)
        self.device = self.net.device
        shp = self.net.output_shapes(1)
        outs = self.net.structure['outputs']
        want = [(1, 512, 1), (1, 384, 1), (1, 512, 16), (1, 384, 16), (1, 16, 16, 3), (1, 8, 8, 3)]
        if [shp[o] for o in outs] != want:
            raise ValueError('unified model outputs %s do not match the BlazeFace front detector %s'
                             % ([shp[o] for o in outs], want))

    def postprocess(self, outs):
        """outs: the six device outputs of the unified graph -> device result tensors."""
        n = outs[0].shape[0]
        M = self.max_faces
        dev = self.device
        count = torch.zeros(n, dtype=torch.int32, device=dev)
        det = torch.empty((n, M), dtype=torch.int32, device=dev)
        scores = torch.empty((n, M), dtype=torch.float32, device=dev)
        boxes = torch.empty((n, M, 4), dtype=torch.float64, device=dev)
        kps = torch.empty((n, M, KEY_POINT_SIZE, 2), dtype=torch.float64, device=dev)
        poses = torch.empty((n, M, 3), dtype=torch.float32, device=dev)
        lib = _lib.load()
        o = [x.contiguous() for x in outs]
        _lib.check(lib.hpe_detect(_ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(o[4]), _ptr(o[5]), n,
                                  float(np.float32(self.sigmoidScoreThreshold)), float(self.iouThreshold), M,
                                  _ptr(count), _ptr(det), _ptr(scores), _ptr(boxes), _ptr(kps), _ptr(poses),
                                  _lib.stream()), 'hpe_detect')
        return dict(count=count, det_index=det, scores=scores, boxes=boxes, keypoints=kps, poses=poses)

    def _results(self, x):
        """x: (n, 128, 128, 3) device model input -> [Results] * n on the host."""
        return _host_results(self.postprocess(self.net.forward(x)))

    def prepare(self, images, bgr=True, crop=None):
        """uint8 frames (H, W, 3) / (n, H, W, 3), or an NV12Frames -> the device model input
        (hpe.preprocess)."""
        return prepare_input(images, size=tuple(self.net.structure['input_hw']), bgr=bgr, crop=crop,
                             device=self.device)

    def detect_images(self, images, bgr=True, crop=None):
        """images: raw uint8 frames (H, W, 3) or (n, H, W, 3), BGR unless bgr=False (numpy or
        tensor, host or device); crop as hpe.preprocess.prepare_input -> [Results] * n.  Here and in
        every method below that takes raw frames, an hpe.preprocess.NV12Frames (decoded video) stands
        for the BGR frames it converts to; bgr=False is refused with one."""
        return self._results(self.prepare(images, bgr=bgr, crop=crop))

    def detect_batch(self, frames):
        """frames: (n, 128, 128, 3) preprocessed input (numpy or device tensor), or raw uint8 frames
        (detect_images) -> [Results] * n."""
        if is_uint8(frames):
            return self.detect_images(frames)
        return self._results(_device_input(frames, self.device))

    def detect_rois(self, frames, rois, bgr=True, pad_value=0):
        """frames: raw uint8 frames; rois: (m, 5) rows of (frame, x0, y0, w, h) in frame pixels, which
        may reach outside the frame (``pad_value`` there), as hpe.preprocess.prepare_rois -> [Results]
        * m, boxes and keypoints normalised to each ROI: what detect_batch returns for the prepared
        ROI images."""
        x = prepare_rois(frames, rois, size=tuple(self.net.structure['input_hw']), bgr=bgr,
                         pad_value=pad_value, device=self.device)
        return self._results(x) if x.shape[0] else []

    def face_rois(self, r, src, scale):
        """r: postprocess() outputs; src: the first pass's source rectangle (x0, y0, w, h) in frame
        pixels -> (rois (n * max_faces, 5) int32, n_rois (1,) int32) on the device (hpe_face_rois): an
        enlarged square around every face, frame-major in NMS order."""
        n = r['count'].shape[0]
        rois = torch.empty((n * self.max_faces, 5), dtype=torch.int32, device=self.device)
        n_rois = torch.zeros(1, dtype=torch.int32, device=self.device)
        _launch('hpe_face_rois', self.device, _ptr(r['count']), _ptr(r['boxes']), n, self.max_faces, int(src[0]),
                int(src[1]), int(src[2]), int(src[3]), float(scale), _ptr(rois), _ptr(n_rois))
        return rois, n_rois

    def detect_refine(self, frames, scale, bgr=True, crop=None, pad_value=0):
        """Detect, then look again at an enlarged square around every face: the first pass as
        detect_images, the ROI table on the device (side = scale x the box's longer side in frame
        pixels; ``scale`` has no measured default), one host read of the ROI count, the second pass
        as detect_rois.  Returns one Results per frame with the first pass's faces in the first
        pass's order.  Where the second pass found anything in a face's ROI, its top-scoring detection
        replaces score, pose, box and keypoints (mapped back to the first pass's normalisation, in
        float64 on the host) and ``refined`` is True; otherwise the first-pass values stay."""
        x, _ = _device_frames(_checked_frames(frames, 'detect_refine', bgr), self.device, None, 'detect_refine')
        _, h, w = frame_dims(x)
        src = crop_rect(h, w, crop)
        r = self.postprocess(self.net.forward(self.prepare(x, bgr=bgr, crop=crop)))
        rois, n_rois = self.face_rois(r, src, scale)
        m = int(n_rois.item())
        res = _host_results(r, copy=True)
        second = self.detect_rois(x, rois[:m], bgr=bgr, pad_value=pad_value) if m else []
        table = rois[:m].cpu().numpy()
        row = 0
        for out in res:
            for j in range(len(out.scores)):
                fr, rx, ry, side, _ = (int(v) for v in table[row])
                s2 = second[row]
                row += 1
                if fr < 0 or not len(s2.scores):
                    continue
                out.scores[j] = s2.scores[0]
                out.poses[j] = s2.poses[0]
                out.boxes[j] = remap_roi(s2.boxes[0].reshape(2, 2), rx, ry, side, src).reshape(4)
                out.keypoints[j] = remap_roi(s2.keypoints[0], rx, ry, side, src)
                out.refined[j] = True
        return res

    def merge_rois(self, r, rois, rows_per_frame, dst, max_faces=None):
        """r: postprocess()'s dict for the ROI images of ``rois``, a frame-major (n * rows_per_frame, 5)
        table (hpe.preprocess.tile_rois); dst: the rectangle (x0, y0, w, h) in frame pixels to normalise
        to -> dict of device tensors count (n,), src, scores (n, max_faces), boxes, keypoints, poses:
        per frame, all its rows' detections remapped to dst and merged by one NMS (hpe_merge_rois),
        in selection order; src = row * max_faces_in + slot.  Slots past count are not written."""
        R = int(rows_per_frame)
        M = r['scores'].shape[1]
        K = self.max_faces if max_faces is None else int(max_faces)
        if R * M > MERGE_MAX_CAND:
            raise ValueError('merge_rois: rows_per_frame %d x max_faces %d exceeds %d candidates per frame'
                             % (R, M, MERGE_MAX_CAND))
        t = roi_table(rois).to(self.device).contiguous()
        if R < 1 or t.shape[0] % R or t.shape[0] != r['count'].shape[0]:
            raise ValueError('merge_rois: %d table rows, %d ROI images, %d rows per frame'
                             % (t.shape[0], r['count'].shape[0], R))
        n = t.shape[0] // R
        dev = self.device
        out = dict(count=torch.zeros(n, dtype=torch.int32, device=dev),
                   src=torch.empty((n, K), dtype=torch.int32, device=dev),
                   scores=torch.empty((n, K), dtype=torch.float32, device=dev),
                   boxes=torch.empty((n, K, 4), dtype=torch.float64, device=dev),
                   keypoints=torch.empty((n, K, KEY_POINT_SIZE, 2), dtype=torch.float64, device=dev),
                   poses=torch.empty((n, K, 3), dtype=torch.float32, device=dev))
        _launch('hpe_merge_rois', dev, _ptr(t), n, R, _ptr(r['count']), _ptr(r['scores']), _ptr(r['boxes']),
                _ptr(r['keypoints']), _ptr(r['poses']), M, int(dst[0]), int(dst[1]), int(dst[2]), int(dst[3]),
                float(self.iouThreshold), K, _ptr(out['count']), _ptr(out['src']), _ptr(out['scores']),
                _ptr(out['boxes']), _ptr(out['keypoints']), _ptr(out['poses']))
        return out

    def detect_tiled(self, frames, tile, overlap=None, full=True, bgr=True, crop=None, pad_value=0, max_faces=None,
                     roi_batch=2048):
        """Look at every frame as a whole (``full``: what detect_images(crop=) sees) and in square tiles
        of ``tile`` frame pixels overlapping by ``overlap`` (None: tile // 4), and merge what all the
        looks found: tile_rois -> prepare_rois -> the network -> postprocess -> merge_rois, with no host
        read before the one copy of the merged results.  Returns one Results per frame, boxes and
        keypoints normalised as detect_images(crop=) returns them, at most ``max_faces`` (None:
        self.max_faces) per frame, with ``roi`` the table row each face came from (0: the whole look
        when full) and ``src`` = row * self.max_faces + slot.  Batches of more than ``roi_batch`` ROI
        images run in chunks of whole frames.  A mechanism, not a policy: a face cut by a tile border
        gives a partial box that only the overlap and the whole look can outvote; no border rule is
        applied and ``tile`` has no measured default."""
        x = _checked_frames(frames, 'detect_tiled', bgr)
        if not isinstance(x, NV12Frames) and x.ndim == 3:
            x = x[None]
        n, h, w = frame_dims(x)
        if overlap is None:
            overlap = tile // 4 if tile is not None else 0
        table, R = tile_rois(n, h, w, tile, overlap, crop=crop, full=full)
        if R * self.max_faces > MERGE_MAX_CAND:
            raise ValueError('detect_tiled: %d rows per frame x max_faces %d exceeds %d candidates per frame'
                             % (R, self.max_faces, MERGE_MAX_CAND))
        if int(roi_batch) < 1:
            raise ValueError('detect_tiled: roi_batch must be positive, got %r' % (roi_batch,))
        if n == 0:
            return []
        x, _ = _device_frames(x, self.device, None, 'detect_tiled')
        dst = crop_rect(h, w, crop)
        step = max(1, int(roi_batch) // R)          # whole frames per chunk
        # a chunk's frames are numbered from 0, so every chunk reads the head of the one table
        t = torch.from_numpy(table[:min(step, n) * R]).to(self.device)
        parts = []
        for f0 in range(0, n, step):
            k = min(step, n - f0)
            imgs = prepare_rois(x[f0:f0 + k], t[:k * R], size=tuple(self.net.structure['input_hw']), bgr=bgr,
                                pad_value=pad_value, device=self.device)
            parts.append(self.merge_rois(self.postprocess(self.net.forward(imgs)), t[:k * R], R, dst, max_faces))
        m = {key: torch.cat([p[key] for p in parts]).cpu().numpy() for key in parts[0]}
        res = []
        for i, c in enumerate(int(c) for c in m['count']):
            out = Results(m['boxes'][i, :c], m['keypoints'][i, :c], m['scores'][i, :c],
                          m['poses'][i, :c] if c else np.zeros((0, 3), np.float32))
            out.src = m['src'][i, :c]
            out.roi = out.src // np.int32(self.max_faces)
            res.append(out)
        return res

    def detect_video(self, frames, tracker, bgr=True, crop=None):
        """frames: raw uint8 frames (T, H, W, 3), the next T frames of one video, or (S, T, H, W, 3), the
        next T frames of each of tracker.streams = S videos (an NV12Frames: y (T, H, W) or (S, T, H, W));
        tracker: a hpe.tracking.PoseTracker, which
        holds the tracks between calls, so consecutive calls continue the same videos.  prepare -> the
        network -> postprocess -> tracker.update, one copy to the host at the end.  Returns T Results
        (a list of S such lists for the 5-d form) as detect_images(bgr=, crop=) returns them, with
        ``track`` the face's id (-1: untracked) and boxes, keypoints and poses smoothed per track."""
        nv12 = isinstance(frames, NV12Frames)
        x = frames if nv12 or torch.is_tensor(frames) else np.asarray(frames)
        lead = x.lead if nv12 else tuple(x.shape[:-3])
        multi = len(lead) == 2
        if len(lead) not in (1, 2):
            raise ValueError('detect_video: frames must be (T, H, W, 3) or (S, T, H, W, 3) (an NV12Frames: y (T, H, W) '
                             'or (S, T, H, W)), got %s' % (tuple((x.y if nv12 else x).shape),))
        S, T = (lead[0], lead[1]) if multi else (1, lead[0])
        if S != tracker.streams:
            raise ValueError('detect_video: %d videos for a tracker of %d streams' % (S, tracker.streams))
        x = _checked_frames(x.flat() if nv12 else x.reshape((S * T,) + tuple(x.shape[-3:])), 'detect_video', bgr)
        if T == 0:
            return [[] for _ in range(S)] if multi else []
        r = tracker.update(self.postprocess(self.net.forward(self.prepare(x, bgr=bgr, crop=crop))))
        track = r.pop('track').cpu().numpy()
        res = _host_results(r)
        for i, out in enumerate(res):
            out.track = track[i, :len(out.scores)]
        return [res[s * T:(s + 1) * T] for s in range(S)] if multi else res

    def draw(self, frames, results, bgr=True, crop=None, style=None):
        """Draw every face's box, keypoints and pose axes into the frames (the reference's drawDetections,
        :175-219, without its text).  frames: raw uint8 frames (H, W, 3) / (n, H, W, 3), BGR unless
        bgr=False, or an NV12Frames.  results: the device dict of postprocess, merge_rois or
        PoseTracker.update for the n frames (nothing is read on the host), or the list of host Results a
        detect_* method returned (packed and uploaded).  crop: as in detect_images, the rectangle the
        detections are normalised to.  style: a hpe.draw.DrawStyle (None: the reference's sizes and
        colours; for NV12 the colours are converted to Y, U, V by hpe.draw.bgr_to_yuv).  Device frames
        are annotated in place and returned; host frames are copied to the device, annotated and
        returned as a new array of the same kind (an NV12Frames gives an NV12Frames)."""
        style = DrawStyle() if style is None else style
        x = _checked_frames(frames, 'draw', bgr)
        nv12 = isinstance(x, NV12Frames)
        on_device = all(torch.is_tensor(p) and p.is_cuda for p in ((x.y, x.uv) if nv12 else (x,)))
        d = x if on_device else _device_frames(x, self.device, None, 'draw')[0]
        n, h, w = frame_dims(d)
        if isinstance(results, dict):
            r = results
        else:
            res = [results] if isinstance(results, Results) else list(results)
            r = {k: torch.from_numpy(v).to(self.device) for k, v in pack_results(res).items()}
        if r['count'].shape[0] != n:
            raise ValueError('draw: results for %d frames, %d frames' % (r['count'].shape[0], n))
        prims, n_prims = pose_prims(r, crop_rect(h, w, crop), style)
        draw_prims(d, prims, n_prims, torch.from_numpy(style.colours(bgr=bgr, nv12=x.matrix if nv12 else None)))
        if on_device:
            return frames
        if nv12:
            y, uv = d.y.cpu(), d.uv.cpu()
            return NV12Frames(y, uv, x.matrix) if torch.is_tensor(x.y) else NV12Frames(y.numpy(), uv.numpy(), x.matrix)
        out = d.cpu() if x.ndim == 4 else d[0].cpu()
        return out if torch.is_tensor(x) else out.numpy()

    def drawDetections(self, img, results):
        """The reference's call (:175): one host BGR frame (H, W, 3) and its Results, drawn into ``img``,
        which is returned.  The reference's text is not drawn."""
        img[...] = self.draw(img, [results])
        return img

    def detectFaces(self, frame):
        if is_uint8(frame):
            return self.detect_images(frame)[0]
        f = np.asarray(frame, np.float32)
        if f.ndim == 3:
            f = f[None]
        return self.detect_batch(f)[0]
