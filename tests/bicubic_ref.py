"""Restatement of the detector's input preparation (prepareInputForInference,
BlazePoser/blazeFaceDetectorH5.py:247-269) that csrc/hpe_preproc.hip must equal bit for bit.

The resize is TF 2.x ResizeBicubic with half_pixel_centers=True (tf.image.resize(method='bicubic')
without antialias): a 1025-entry Keys cubic (A = -0.5) weight table indexed by the fractional source
location in 1/1024 steps, taps clamped to the image, a clamped tap's weight set to 0 and the rest
divided by their sum, the y pass first and the x pass on its four columns.  Everything is vectorised
float32 NumPy: each elementwise op rounds once, exactly as the kernel's separately rounded ops.
``weights_f64`` / ``resize_f64`` evaluate the same taps and table offsets in float64 (a scalar loop
for the weights) to bound the fp32 rounding.

TensorFlow is not available here: this is the arithmetic of TF's kernel written out and checked
against Pillow where the two agree (upscales of float images), not against TF output.
"""
import numpy as np

F = np.float32
TABLE = 1024
A = F(-0.5)
FLT_MIN = np.finfo(np.float32).tiny


def coeffs():
    """TF's coefficient table: near[i] (|x| <= 1) and far[i] (1 < |x| < 2) at x = i / 1024."""
    t = (np.arange(TABLE + 1) / 1024.0).astype(F)
    near = ((A + F(2)) * t - (A + F(3))) * t * t + F(1)
    u = t + F(1)
    far = ((A * u - F(5) * A) * u + F(8) * A) * u - F(4) * A
    assert near.dtype == F and far.dtype == F
    return near, far


def locate(out_size, in_size):
    """Per output index: floor of the source location (int64) and the table offset 0..1024, by
    the fp32 rule (loc_f = (o + 0.5) * scale - 0.5, ties of the offset to even)."""
    scale = F(in_size) / F(out_size)
    o = np.arange(out_size).astype(F)
    loc_f = (o + F(0.5)) * scale - F(0.5)
    loc = np.floor(loc_f)
    d = loc_f - loc
    off = np.rint(d * F(1024)).astype(np.int64)
    assert loc_f.dtype == F and d.dtype == F
    return loc.astype(np.int64), off


def weights(out_size, in_size):
    """-> (index (out, 4) int64 clamped to the image, weight (out, 4) float32)."""
    near, far = coeffs()
    loc, off = locate(out_size, in_size)
    raw = loc[:, None] + np.arange(-1, 3)[None, :]
    idx = np.clip(raw, 0, in_size - 1)
    w = np.stack([far[off], near[off], near[TABLE - off], far[TABLE - off]], axis=1)
    w = np.where(idx == raw, w, F(0))
    s = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    ok = np.abs(s) >= F(1000) * FLT_MIN
    inv = F(1) / np.where(ok, s, F(1))
    w = np.where(ok[:, None], w * inv[:, None], w)
    assert w.dtype == F
    return idx, w


def weights_f64(out_size, in_size):
    """The same taps and table offsets, weights evaluated and normalised in float64 (scalar loop)."""
    loc, off = locate(out_size, in_size)
    a = -0.5
    idx = np.zeros((out_size, 4), np.int64)
    w = np.zeros((out_size, 4), np.float64)

    def near(t):
        return ((a + 2) * t - (a + 3)) * t * t + 1

    def far(t):
        u = t + 1
        return ((a * u - 5 * a) * u + 8 * a) * u - 4 * a

    for o in range(out_size):
        t0, t1 = int(off[o]) / 1024.0, (TABLE - int(off[o])) / 1024.0
        ws = [far(t0), near(t0), near(t1), far(t1)]
        for k in range(4):
            i = int(loc[o]) - 1 + k
            c = min(max(i, 0), in_size - 1)
            idx[o, k] = c
            w[o, k] = ws[k] if c == i else 0.0
        s = ((w[o, 0] + w[o, 1]) + w[o, 2]) + w[o, 3]
        if abs(s) >= 1000 * float(FLT_MIN):
            w[o] *= 1.0 / s
    return idx, w


def _interp(img, yi, wy, xi, wx):
    v = img[:, yi[:, :, None, None], xi[None, None, :, :]]          # (n, oh, 4, ow, 4, C)
    wy = wy[None, :, :, None, None, None]
    c = ((v[:, :, 0] * wy[:, :, 0] + v[:, :, 1] * wy[:, :, 1]) + v[:, :, 2] * wy[:, :, 2]) + v[:, :, 3] * wy[:, :, 3]
    wx = wx[None, None, :, :, None]                                  # c: (n, oh, ow, 4, C)
    return ((c[:, :, :, 0] * wx[:, :, :, 0] + c[:, :, :, 1] * wx[:, :, :, 1]) + c[:, :, :, 2] * wx[:, :, :, 2]) \
        + c[:, :, :, 3] * wx[:, :, :, 3]


def resize(img, out_h, out_w):
    """img (n, H, W, C) float32 -> (n, out_h, out_w, C) float32, every op a rounded fp32 op."""
    img = np.asarray(img)
    assert img.dtype == F and img.ndim == 4
    yi, wy = weights(out_h, img.shape[1])
    xi, wx = weights(out_w, img.shape[2])
    r = _interp(img, yi, wy, xi, wx)
    assert r.dtype == F
    return r


def resize_f64(img, out_h, out_w):
    img = np.asarray(img, np.float64)
    yi, wy = weights_f64(out_h, img.shape[1])
    xi, wx = weights_f64(out_w, img.shape[2])
    return _interp(img, yi, wy, xi, wx)


def crop_rect(h, w, crop):
    """None / 'square' (the webcam loop's centre crop, :394-399) / (x0, y0, w, h) -> (x0, y0, w, h)."""
    if crop is None:
        return 0, 0, w, h
    if isinstance(crop, str):
        assert crop == 'square'
        side = min(h, w)
        return (w - side) // 2, (h - side) // 2, side, side
    return tuple(int(c) for c in crop)


def tap_values(frames, bgr=True, crop=None):
    """uint8 (n, H, W, 3) -> the cropped float32 RGB image in [0, 1]: (float)(byte / 255.0)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4
    x0, y0, cw, ch = crop_rect(frames.shape[1], frames.shape[2], crop)
    u8 = frames[:, y0:y0 + ch, x0:x0 + cw]
    if bgr:
        u8 = u8[..., ::-1]
    lut = (np.arange(256) / 255.0).astype(F)
    return lut[u8]


def preprocess(frames, size=128, bgr=True, crop=None):
    """uint8 frames (n, H, W, 3) -> (n, h, w, 3) float32 network input, the kernel's exact bits."""
    h, w = (size, size) if np.isscalar(size) else size
    r = resize(tap_values(frames, bgr, crop), int(h), int(w))
    r = (r - F(0.5)) / F(0.5)
    assert r.dtype == F
    return r


def preprocess_f64(frames, size=128, bgr=True, crop=None):
    h, w = (size, size) if np.isscalar(size) else size
    return (resize_f64(tap_values(frames, bgr, crop), int(h), int(w)) - 0.5) / 0.5
