"""Restatement of the per-ROI frame preparation (hpe_preprocess_rois) and of the second-pass ROI table
(hpe_face_rois) that the kernels of csrc/hpe_preproc.hip must equal exactly.

The preparation goes the canvas route: the ROI's h x w canvas is built with numpy (frame pixels where
the ROI overlaps the frame, the pad bytes elsewhere) and handed whole to bicubic_ref.preprocess, so
the taps clamp to the canvas.  The ROI table is the issue's arithmetic in numpy float64, one rounded
operation per numpy call.
"""
import numpy as np

import bicubic_ref as B

LIM = 1 << 24
INVALID = (-1, 0, 0, 0, 0)


def pad3(pad_value):
    return (int(pad_value),) * 3 if np.isscalar(pad_value) else tuple(int(v) for v in pad_value)


def valid(roi, n_frames):
    """The device's rule for a row (frame, x0, y0, w, h)."""
    f, x0, y0, w, h = (int(v) for v in roi)
    return 0 <= f < n_frames and 1 <= w <= LIM and 1 <= h <= LIM and abs(x0) <= LIM and abs(y0) <= LIM


def canvas(frame, x0, y0, w, h, pad_value=0):
    """uint8 (H, W, 3) frame -> the (h, w, 3) canvas whose pixel (y, x) is frame[y0 + y, x0 + x] inside
    the frame and the pad bytes (frame channel order) elsewhere."""
    H, W, _ = frame.shape
    c = np.empty((h, w, 3), np.uint8)
    c[:] = np.asarray(pad3(pad_value), np.uint8)
    ya, yb = max(y0, 0), min(y0 + h, H)
    xa, xb = max(x0, 0), min(x0 + w, W)
    if ya < yb and xa < xb:
        c[ya - y0:yb - y0, xa - x0:xb - x0] = frame[ya:yb, xa:xb]
    return c


def pad_constant(size, bgr=True, pad_value=0):
    """An invalid row's output: (lut[pad_c] - 0.5f) / 0.5f per channel, after the bgr swap."""
    oh, ow = (size, size) if np.isscalar(size) else size
    p = np.asarray(pad3(pad_value), np.uint8)
    if bgr:
        p = p[::-1]
    lut = (np.arange(256) / 255.0).astype(B.F)
    v = (lut[p] - B.F(0.5)) / B.F(0.5)
    assert v.dtype == B.F
    return np.broadcast_to(v, (int(oh), int(ow), 3)).copy()


def prepare_rois(frames, rois, size=128, bgr=True, pad_value=0):
    """uint8 (n, H, W, 3) frames, (m, 5) rows -> (m, oh, ow, 3) float32, the kernel's exact bits."""
    frames = np.asarray(frames)
    oh, ow = (size, size) if np.isscalar(size) else size
    out = np.empty((len(rois), int(oh), int(ow), 3), B.F)
    for r, roi in enumerate(rois):
        if valid(roi, len(frames)):
            f, x0, y0, w, h = (int(v) for v in roi)
            out[r] = B.preprocess(canvas(frames[f], x0, y0, w, h, pad_value)[None], size, bgr=bgr)[0]
        else:
            out[r] = pad_constant(size, bgr, pad_value)
    return out


def face_rois(count, boxes, src, scale):
    """count (n,), boxes (n, M, 4) float64 [x1, y1, x2, y2] normalised to src = (x0, y0, w, h) ->
    (rois (n * M, 5) int32, n_rois): an S x S square per detection, frame-major in detection order,
    the rows past n_rois invalid."""
    boxes = np.asarray(boxes, np.float64)
    n, M, _ = boxes.shape
    sx0, sy0, sw, sh = (np.float64(v) for v in src)
    scale = np.float64(scale)
    rois = np.tile(np.asarray(INVALID, np.int32), (n * M, 1))
    k = 0
    lim = np.float64(LIM)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            for j in range(min(max(int(count[i]), 0), M)):
                x1, y1, x2, y2 = boxes[i, j]
                px1, py1 = sx0 + x1 * sw, sy0 + y1 * sh
                px2, py2 = sx0 + x2 * sw, sy0 + y2 * sh
                cx, cy = np.float64(0.5) * (px1 + px2), np.float64(0.5) * (py1 + py2)
                side = scale * np.fmax(px2 - px1, py2 - py1)
                if np.isfinite(cx) and np.isfinite(cy) and np.isfinite(side):
                    S = np.clip(np.ceil(side), 1.0, lim)
                    rx = np.clip(np.floor(cx - np.float64(0.5) * S), -lim, lim)
                    ry = np.clip(np.floor(cy - np.float64(0.5) * S), -lim, lim)
                    rois[k] = (i, int(rx), int(ry), int(S), int(S))
                k += 1
    return rois, k


def remap(xy, roi, src):
    """(..., 2) float64 points normalised to the square ROI row -> normalised to src."""
    _, rx, ry, S, _ = (int(v) for v in roi)
    xy = np.asarray(xy, np.float64)
    X = (rx + xy[..., 0] * S - src[0]) / src[2]
    Y = (ry + xy[..., 1] * S - src[1]) / src[3]
    return np.stack([X, Y], -1)
