"""Detections and pose axes drawn into video frames on the device: ``drawDetections`` of
BlazePoser/blazeFaceDetectorH5.py:175-219 (with ``drawAxis_simo`` :64-77 and ``EulerToMatrix`` :40-62),
the last stage of the reference's webcam loop, without a copy of the frame to the host
(csrc/hpe_draw.hip, C ABI ``hpe_pose_prims``, ``hpe_draw``, ``hpe_draw_nv12``; the rules are written
out in include/hpe.h).

Two stages.  ``pose_prims`` turns the device results of the detector, the merge or the tracker into a
table of integer primitives, 11 rows per face: the box outline, six keypoint disks and the three pose
axes.  ``draw_prims`` rasterises any such table into packed 3-byte frames or NV12 planes in place, so
it serves any overlay made of rectangle outlines, disks and thick segments.  Not drawn: the reference's
text (score, angles, FPS: it needs OpenCV's font data); no anti-aliasing, no alpha blending.  The
coverage rules are this project's; their parity with OpenCV's rasterisation is unpinned.
"""
import numpy as np
import torch

from ._lib import ptr as _ptr
from .preprocess import NV12Frames, _checked_frames, _launch, frame_dims

PRIM_WORDS = 8    # HPE_DRAW_PRIM_WORDS
FACE_PRIMS = 11   # HPE_DRAW_FACE_PRIMS
MAX_DIM = 8192    # HPE_DRAW_MAX_DIM
MAX_SIZE = 64     # HPE_DRAW_MAX_SIZE
RECT, DISK, SEGMENT = 1, 2, 3   # the primitive kinds

# round(256 c) of the limited-range RGB -> YCbCr matrices, rows Y, U, V over (R, G, B)
YUV_MATRICES = {'bt601': ((66, 129, 25), (-38, -74, 112), (112, -94, -18)),
                'bt709': ((47, 157, 16), (-26, -87, 112), (112, -102, -10))}


def bgr_to_yuv(bgr, matrix='bt601'):
    """One BGR colour -> (Y, U, V) bytes: ((row . (R, G, B) + 128) >> 8) + 16 for Y, + 128 for U and V,
    with the integer rows of YUV_MATRICES (>> is a floor).  Agreement with any encoder's conversion is
    unpinned."""
    if matrix not in YUV_MATRICES:
        raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
    b, g, r = (int(c) for c in bgr)
    return tuple(min(max(((m[0] * r + m[1] * g + m[2] * b + 128) >> 8) + o, 0), 255)
                 for m, o in zip(YUV_MATRICES[matrix], (16, 128, 128)))


class DrawStyle:
    """What drawDetections draws and how; the defaults are the reference's (:190, :198, :73-75).  Colours
    are BGR; a thickness of 0, or ``box`` / ``keypoints`` / ``axes`` False, leaves that part out."""

    def __init__(self, box_thickness=2, box_colour=(22, 22, 250), keypoint_radius=4, keypoint_colour=(214, 202, 18),
                 axis_colours=((0, 255, 0), (0, 0, 255), (255, 0, 0)), axis_thickness=(3, 3, 2), box=True,
                 keypoints=True, axes=True):
        self.box_thickness = int(box_thickness)
        self.box_colour = tuple(box_colour)
        self.keypoint_radius = int(keypoint_radius)
        self.keypoint_colour = tuple(keypoint_colour)
        self.axis_colours = tuple(tuple(c) for c in axis_colours)
        self.axis_thickness = tuple(int(t) for t in axis_thickness)
        self.box, self.keypoints, self.axes = bool(box), bool(keypoints), bool(axes)
        cols = (self.box_colour, self.keypoint_colour) + self.axis_colours
        if len(self.axis_colours) != 3 or len(self.axis_thickness) != 3 or any(
                len(c) != 3 or any(not 0 <= int(v) <= 255 for v in c) for c in cols):
            raise ValueError('DrawStyle: three axis colours and thicknesses, colours of three bytes')

    def sizes(self):
        """(box_th, kp_radius, axis_th_x, axis_th_y, axis_th_z) as hpe_pose_prims takes them."""
        ax = self.axis_thickness if self.axes else (0, 0, 0)
        return (self.box_thickness if self.box else 0, self.keypoint_radius if self.keypoints else -1) + tuple(ax)

    def colours(self, bgr=True, nv12=None):
        """The colour table of hpe_pose_prims' indices (0 box, 1 keypoint, 2 / 3 / 4 the axes): (5, 4)
        uint8, byte 3 zero.  bgr=False swaps bytes 0 and 2 (RGB frames); nv12 ('bt601' or 'bt709'):
        (Y, U, V) bytes for NV12Frames of that matrix (bgr_to_yuv)."""
        t = np.zeros((5, 4), np.uint8)
        for i, c in enumerate((self.box_colour, self.keypoint_colour) + self.axis_colours):
            t[i, :3] = bgr_to_yuv(c, nv12) if nv12 is not None else (c if bgr else c[::-1])
        return t


def pose_prims(r, src, style=None):
    """r: the device dict of BlazeFaceDetector.postprocess, merge_rois or PoseTracker.update (count,
    boxes, keypoints, poses); src: the rectangle (x0, y0, w, h) in frame pixels the detections are
    normalised to.  Returns (prims (n, 11 * max_faces, 8) int32, n_prims (n,) int32) on the device
    (hpe_pose_prims).  No host read."""
    style = DrawStyle() if style is None else style
    dev = r['boxes'].device
    n, M = r['boxes'].shape[0], r['boxes'].shape[1]
    count = r['count'].to(dev, torch.int32).contiguous()
    boxes = r['boxes'].to(dev, torch.float64).contiguous()
    kps = r['keypoints'].to(dev, torch.float64).contiguous()
    poses = r['poses'].to(dev, torch.float32).contiguous()
    prims = torch.zeros((n, FACE_PRIMS * M, PRIM_WORDS), dtype=torch.int32, device=dev)
    n_prims = torch.zeros(n, dtype=torch.int32, device=dev)
    _launch('hpe_pose_prims', dev, _ptr(count), _ptr(boxes), _ptr(kps), _ptr(poses), n, M, int(src[0]), int(src[1]),
            int(src[2]), int(src[3]), *style.sizes(), _ptr(prims), _ptr(n_prims))
    return prims, n_prims


def draw_prims(frames, prims, n_prims, colours):
    """Rasterise the table into ``frames`` in place (hpe_draw / hpe_draw_nv12): a device uint8
    (n, H, W, 3) tensor, written through its row stride, or an NV12Frames of device planes, written
    through their strides.  prims (n, P, 8) int32, n_prims (n,) int32, colours (k, 4) uint8, k <= 256 (for
    NV12 the bytes are Y, U, V).  Frames that cannot be written in place (host arrays, device tensors
    whose pixels are not contiguous) are refused: BlazeFaceDetector.draw copies them.  Returns frames."""
    x = _checked_frames(frames, 'draw_prims')
    nv12 = isinstance(x, NV12Frames)
    planes = (x.y, x.uv) if nv12 else (x if x.ndim == 4 else x[None],)
    if not all(torch.is_tensor(p) and p.is_cuda for p in planes):
        raise ValueError('draw_prims writes device frames in place; BlazeFaceDetector.draw copies host frames')
    n, h, w = frame_dims(x)
    px = 1 if nv12 else 3   # bytes per pixel of a row
    if any(tuple(p.stride()[2:]) != ((1,) if nv12 else (3, 1)) or p.stride(1) < px * w for p in planes):
        raise ValueError('draw_prims: the frames cannot be written in place (pixels not contiguous, or rows that '
                         'overlap)')
    dev = planes[0].device
    prims = prims.to(dev, torch.int32).contiguous()
    n_prims = n_prims.to(dev, torch.int32).contiguous()
    colours = torch.as_tensor(colours).to(dev, torch.uint8).contiguous()
    if prims.dim() != 3 or prims.shape[0] != n or prims.shape[2] != PRIM_WORDS or tuple(n_prims.shape) != (n,):
        raise ValueError('draw_prims: prims %s / n_prims %s do not fit %d frames' % (tuple(prims.shape),
                                                                                    tuple(n_prims.shape), n))
    if colours.dim() != 2 or colours.shape[1] != 4:
        raise ValueError('draw_prims: colours must be (k, 4) uint8, got %s' % (tuple(colours.shape),))
    if nv12:
        y, uv = planes
        _launch('hpe_draw_nv12', dev, _ptr(y), _ptr(uv), n, h, w, y.stride(1), y.stride(0), uv.stride(1), uv.stride(0),
                _ptr(prims), _ptr(n_prims), prims.shape[1], _ptr(colours), colours.shape[0])
    else:
        p = planes[0]
        _launch('hpe_draw', dev, _ptr(p), n, h, w, p.stride(1), p.stride(0), _ptr(prims), _ptr(n_prims),
                prims.shape[1], _ptr(colours), colours.shape[0])
    return frames


def pack_results(results, max_faces=None):
    """[Results] * n (host) -> the host dict of numpy arrays count (n,), boxes (n, M, 4), keypoints
    (n, M, 6, 2), poses (n, M, 3) that pose_prims takes once uploaded; M: max_faces, or the longest list."""
    n = len(results)
    M = max([1] + [len(r.scores) for r in results]) if max_faces is None else int(max_faces)
    out = dict(count=np.zeros(n, np.int32), boxes=np.zeros((n, M, 4), np.float64),
               keypoints=np.zeros((n, M, 6, 2), np.float64), poses=np.zeros((n, M, 3), np.float32))
    for i, r in enumerate(results):
        c = min(len(r.scores), M)
        out['count'][i] = c
        if c:
            out['boxes'][i, :c] = np.asarray(r.boxes, np.float64).reshape(-1, 4)[:c]
            out['keypoints'][i, :c] = np.asarray(r.keypoints, np.float64).reshape(-1, 6, 2)[:c]
            out['poses'][i, :c] = np.asarray(r.poses, np.float32).reshape(-1, 3)[:c]
    return out
