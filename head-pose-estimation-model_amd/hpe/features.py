"""Feature-dataset extraction on the GPU: regenerate the
``FeatureMaps-Datasets/<set>_features_88_<t>_<k>.npz`` / ``..._96_<t>_<k>.npz`` files the regressors
train on (Model-96/train_96.py:123-130, Model-88/train_88.py:270-280 load them with
``utilities.load_dataset``: keys ``features`` (N, C) float32 and ``poses`` (N, 3) float64).

The extractor itself is outside the reference repo; its interface is pinned by the reference's
files: JoinModels.py:114-116 taps ``re_lu_10`` (16x16x88) and ``re_lu_15`` (8x8x96) of the BlazeFace
front model, and the unified detector reads each detection's pose from the regressor cell of that
detection (BlazePoser/blazeFaceDetectorH5.py:342-353: front anchors d < 512 -> re_lu_10 cell d//2,
back anchors -> re_lu_15 cell (d-512)//6).  A face's feature row is therefore the tap vector the
unified model's regressor consumed for that detection: front detections go to the 88-channel set,
back detections to the 96-channel set, ``<t>`` is the detector score threshold (0.7) and ``<k>`` the
number of faces kept per frame (1).  This is what the dataset sizes show (AFLW2000: 9 rows in the
_88 set + 1809 in the _96 set of 2000 frames).

Pipeline, all on the device: hpe_blazeface_forward (taps written once, in HBM) -> hpe_forward of
the two embedded regressors -> hpe_detect (threshold, decode, NMS) -> hpe_gather_features.  Frames
are either the prepared float model input or raw uint8 camera frames, which hpe_preprocess prepares
on the device first (``prepareInputForInference``, blazeFaceDetectorH5.py:247-269: RGB, /255, bicubic
resize to 128x128, (x - 0.5) / 0.5; hpe.preprocess), batch by batch.  Image decoding is the caller's.

``rois=`` runs the same pipeline on regions of interest of uint8 frames instead of whole frames
(hpe_preprocess_rois): rows (frame, x0, y0, w, h) that may reach outside the frame, ``pad_value``
there.  That is the mechanism for the reference's ``*_Enlarged_features_*`` sets, whose frames were
placed on a larger canvas; what the out-of-repo extractor did exactly (canvas size, pad colour) is
unknown, so their recipe stays unpinned.  Features of an ROI pass are indexed by ROI row.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr
from .detector import BlazeFaceDetector, _device_input, is_uint8
from .preprocess import prepare_rois, roi_table


def _host_rois(rois, crop):
    """extract's ``rois=``, array-like or tensor -> the checked host (m, 5) int32 array, which passes
    through unchanged a second time; None stays None."""
    if rois is None:
        return None
    if crop is not None:
        raise ValueError('rois= takes no crop=')
    return roi_table(rois.cpu() if torch.is_tensor(rois) else rois).numpy()


class FeatureExtractor:
    """``extract(frames)`` -> per-frame device features of the first ``max_faces`` detections;
    ``build_datasets(frames, poses, prefix)`` -> the two .npz files."""

    def __init__(self, model_config, weights, scoreThreshold=0.7, iouThreshold=0.3, max_faces=1,
                 device=None):
        self.det = BlazeFaceDetector(model_config, weights, scoreThreshold=scoreThreshold,
                                     iouThreshold=iouThreshold, device=device, max_faces=max_faces)
        self.scoreThreshold = scoreThreshold
        self.max_faces = int(max_faces)
        net = self.det.net
        st = net.structure
        # the detector's geometry: the taps feeding the 16x16 and the 8x8 pose maps
        by_shape = {}
        for r in st['regressors']:
            th, tw, c = st['shapes'][r['tap']]
            by_shape[(th, tw)] = (r['tap'], c)
        if (16, 16) not in by_shape or (8, 8) not in by_shape:
            raise ValueError('unified model needs regressors on a 16x16 and an 8x8 tap')
        self.tap_front, self.c_front = by_shape[(16, 16)]
        self.tap_back, self.c_back = by_shape[(8, 8)]
        if self.c_front % 4 or self.c_back % 4:
            raise ValueError('tap channels must be multiples of 4')

    @classmethod
    def from_file(cls, path, **kw):
        from .model import load_model
        m = load_model(path, compile=False)
        return cls(m.model_config, m.weights_dict(), **kw)

    def extract_device(self, frames, bgr=True, crop=None, rois=None, pad_value=0):
        """frames (n,128,128,3) prepared float input, or raw uint8 frames (n,H,W,3) or an
        hpe.preprocess.NV12Frames (``bgr`` / ``crop`` as hpe.preprocess.prepare_input) -> dict of
        device tensors: feat88 (n,k,C0), feat96 (n,k,C1),
        src (n,k) int32 (0 front / 1 back / -1 none), plus the detector outputs.  With ``rois`` ((m, 5)
        rows of (frame, x0, y0, w, h), ``pad_value`` outside the frame: hpe.preprocess.prepare_rois)
        the inputs are the m regions of the uint8 frames and n = m."""
        net, dev = self.det.net, self.det.device
        if rois is not None:
            if not is_uint8(frames) or crop is not None:
                raise ValueError('rois= takes raw uint8 frames and no crop=')
            x = prepare_rois(frames, rois, size=tuple(net.structure['input_hw']), bgr=bgr, pad_value=pad_value,
                             device=dev)
        elif is_uint8(frames):
            x = self.det.prepare(frames, bgr=bgr, crop=crop)
        else:
            x = _device_input(frames, dev)
        n = x.shape[0]
        r = self.det.postprocess(net.forward(x))
        k = self.max_faces
        f0 = torch.empty((n, k, self.c_front), dtype=torch.float32, device=dev)
        f1 = torch.empty((n, k, self.c_back), dtype=torch.float32, device=dev)
        src = torch.empty((n, k), dtype=torch.int32, device=dev)
        t0 = net.taps[self.tap_front].contiguous()
        t1 = net.taps[self.tap_back].contiguous()
        lib = _lib.load()
        _lib.check(lib.hpe_gather_features(_ptr(r['count']), _ptr(r['det_index']), n, self.max_faces, k,
                                           _ptr(t0), self.c_front, _ptr(t1), self.c_back, _ptr(f0), _ptr(f1),
                                           _ptr(src), _lib.stream()), 'hpe_gather_features')
        r.update(feat88=f0, feat96=f1, src=src)
        return r

    def _roi_batch(self, frames, rois, bgr, pad_value):
        """One slice of a host ROI table: only the frames its valid rows name are handed on."""
        rois = rois.copy()
        ok = (rois[:, 0] >= 0) & (rois[:, 0] < len(frames))
        rois[~ok, 0] = -1
        lo, hi = (int(rois[ok, 0].min()), int(rois[ok, 0].max()) + 1) if ok.any() else (0, min(1, len(frames)))
        rois[ok, 0] -= lo
        return self.extract_device(frames[lo:hi], bgr=bgr, rois=rois, pad_value=pad_value)

    def extract(self, frames, batch_size=1024, bgr=True, crop=None, rois=None, pad_value=0):
        """Host arrays: (features_front (m0,C0), frame index (m0,), features_back (m1,C1), frame
        index (m1,)) in frame order, detections in NMS order within a frame.  uint8 frames are
        prepared on the device one ``batch_size`` slice at a time.  With ``rois`` (a host (m, 5) table,
        as extract_device) the slices are of ROI rows and the two index arrays are ROI rows."""
        fr, ir, bk, ib = [], [], [], []
        rois = _host_rois(rois, crop)
        n = len(frames) if rois is None else len(rois)
        for s in range(0, n, batch_size):
            if rois is None:
                r = self.extract_device(frames[s:s + batch_size], bgr=bgr, crop=crop)
            else:
                r = self._roi_batch(frames, rois[s:s + batch_size], bgr, pad_value)
            src = r['src'].cpu().numpy()
            f0 = r['feat88'].cpu().numpy()
            f1 = r['feat96'].cpu().numpy()
            i0, j0 = np.nonzero(src == 0)
            i1, j1 = np.nonzero(src == 1)
            fr.append(f0[i0, j0])
            ir.append(i0 + s)
            bk.append(f1[i1, j1])
            ib.append(i1 + s)
        cat = lambda a, c, dt: np.concatenate(a) if a else np.zeros((0,) + c, dt)  # noqa: E731
        return (cat(fr, (self.c_front,), np.float32), cat(ir, (), np.int64),
                cat(bk, (self.c_back,), np.float32), cat(ib, (), np.int64))

    def dataset_names(self, prefix):
        t = ('%g' % self.scoreThreshold)
        return ('%s_features_%d_%s_%d.npz' % (prefix, self.c_front, t, self.max_faces),
                '%s_features_%d_%s_%d.npz' % (prefix, self.c_back, t, self.max_faces))

    def build_datasets(self, frames, poses, prefix, batch_size=1024, bgr=True, crop=None, rois=None,
                       pad_value=0):
        """Write <prefix>_features_88_<t>_<k>.npz and <prefix>_features_96_<t>_<k>.npz (keys
        ``features`` float32, ``poses`` float64 yaw/pitch/roll of the frame); returns the paths.  With
        ``rois`` (as extract) a row's pose is that of the frame its ROI names."""
        poses = np.asarray(poses, np.float64).reshape(-1, 3)
        if len(poses) != len(frames):
            raise ValueError('need one (yaw, pitch, roll) per frame: %d frames, %d poses'
                             % (len(frames), len(poses)))
        rois = _host_rois(rois, crop)
        f0, i0, f1, i1 = self.extract(frames, batch_size, bgr=bgr, crop=crop, rois=rois, pad_value=pad_value)
        if rois is not None:       # ROI rows -> frames; a detection in an invalid row's pad image has no pose
            fr = rois[:, 0]
            k0, k1 = ((fr[i] >= 0) & (fr[i] < len(frames)) for i in (i0, i1))
            f0, i0, f1, i1 = f0[k0], fr[i0][k0], f1[k1], fr[i1][k1]
        p0, p1 = self.dataset_names(prefix)
        d = os.path.dirname(p0)
        if d:
            os.makedirs(d, exist_ok=True)
        np.savez(p0, features=f0, poses=poses[i0])
        np.savez(p1, features=f1, poses=poses[i1])
        return p0, p1
