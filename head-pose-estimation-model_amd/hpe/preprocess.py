"""Raw camera frames -> network input on the GPU: ``prepareInputForInference`` of
BlazePoser/blazeFaceDetectorH5.py:247-269 (cv2.COLOR_BGR2RGB, / 255.0, tf.image.resize(method=
'bicubic'), (x - 0.5) / 0.5) for a batch of uint8 frames in one kernel (csrc/hpe_preproc.hip, C ABI
``hpe_preprocess``), and the same per region of interest (``prepare_rois``, C ABI
``hpe_preprocess_rois``): many rectangles per frame, which may reach outside it; ``tile_rois`` is the
table of tiled detection (the whole look and overlapping square tiles of every frame).  The frames are
uploaded as bytes; everything after the upload stays on the device.  Decoded video arrives as NV12 (a
luma plane and a half-resolution plane of interleaved U, V): ``NV12Frames`` wraps such frames, and
everything that takes uint8 BGR frames takes one and does what it would do for the frames converted to
BGR by the fixed-point rule of include/hpe.h, the conversion happening inside the gather (C ABI
``hpe_preprocess_nv12`` / ``hpe_preprocess_rois_nv12``).  Drawing into such frames is hpe.draw's.  Image
decoding and webcam capture stay out of scope.
"""
import numpy as np
import torch

from . import _lib


def crop_rect(h, w, crop):
    """crop: None (whole frame), 'square' (the webcam loop's centre crop, :394-399) or
    (x0, y0, w, h) -> (x0, y0, w, h)."""
    if crop is None:
        return 0, 0, w, h
    if isinstance(crop, str):
        if crop != 'square':
            raise ValueError("crop must be None, 'square' or (x0, y0, w, h), got %r" % (crop,))
        side = min(h, w)
        return (w - side) // 2, (h - side) // 2, side, side
    if len(crop) != 4:
        raise ValueError("crop must be None, 'square' or (x0, y0, w, h), got %r" % (crop,))
    return tuple(int(c) for c in crop)


MATRICES = {'bt601': 0, 'bt709': 1}     # the `matrix` argument of hpe_preprocess_nv12


def _u8_plane(x, name):
    x = x if torch.is_tensor(x) else np.asarray(x)
    if x.dtype != (torch.uint8 if torch.is_tensor(x) else np.uint8):
        raise ValueError('NV12Frames takes uint8 planes, got %s for %s' % (x.dtype, name))
    return x


class NV12Frames:
    """Decoded NV12 video frames: ``y`` uint8 (H, W) or (n, H, W) (for detect_video also (S, T, H, W)),
    ``uv`` uint8 (..., H/2, W/2, 2) or (..., H/2, W) with the same leading axes, numpy arrays or
    tensors, host or device; with ``uv=None``, ``y`` is the packed (..., 3H/2, W) layout (the Y rows,
    then the UV rows).  The chroma of pixel (y, x) is uv[y >> 1][x >> 1]; ``matrix`` ('bt601' or
    'bt709', both limited range) picks the coefficients of the conversion stated in include/hpe.h.
    H and W must be even.  A device plane whose rows are contiguous is read in place through its
    strides, so a decoder surface with a pitch above W, or two separate allocations, need no copy.
    ``n``, ``h``, ``w``: the number of frames and the luma size; slicing along the first axis gives
    an NV12Frames of the same planes."""

    def __init__(self, y, uv=None, matrix='bt601'):
        if matrix not in MATRICES:
            raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
        y = _u8_plane(y, 'y')
        if y.ndim not in (2, 3, 4):
            raise ValueError('y must be (H, W), (n, H, W) or (S, T, H, W), got %s' % (tuple(y.shape),))
        if uv is None:
            rows = y.shape[-2]
            if rows % 3:
                raise ValueError('a packed NV12 frame has 3H/2 rows, got %d' % rows)
            y, uv = y[..., :rows // 3 * 2, :], y[..., rows // 3 * 2:, :]
        else:
            uv = _u8_plane(uv, 'uv')
        h, w = int(y.shape[-2]), int(y.shape[-1])
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError('an NV12 frame must have an even, positive size, got %d x %d' % (h, w))
        lead = tuple(y.shape[:-2])
        if uv.ndim == y.ndim + 1 and tuple(uv.shape) == lead + (h // 2, w // 2, 2):
            uv = uv.reshape(lead + (h // 2, w))      # a view where the pairs are contiguous
        if tuple(uv.shape) != lead + (h // 2, w):
            raise ValueError('uv must be %s or %s for y %s, got %s' % (lead + (h // 2, w // 2, 2), lead + (h // 2, w),
                                                                     tuple(y.shape), tuple(uv.shape)))
        if not lead:
            y, uv, lead = y[None], uv[None], (1,)
        self.y, self.uv, self.matrix = y, uv, matrix
        self.lead, self.h, self.w = lead, h, w
        self.n = int(np.prod(lead))

    def __len__(self):
        return self.lead[0]

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError('NV12Frames takes slices along the frame axis, got %r' % (key,))
        return NV12Frames(self.y[key], self.uv[key], self.matrix)

    def flat(self):
        """The same frames with one leading axis."""
        if len(self.lead) == 1:
            return self
        return NV12Frames(self.y.reshape((self.n, self.h, self.w)), self.uv.reshape((self.n, self.h // 2, self.w)),
                          self.matrix)

    @property
    def device(self):
        return self.y.device if torch.is_tensor(self.y) else torch.device('cpu')


def frame_dims(x):
    """Checked frames (an NV12Frames, or a uint8 (H, W, 3) / (n, H, W, 3) array or tensor) -> (n, H, W)."""
    if isinstance(x, NV12Frames):
        return x.n, x.h, x.w
    return (x.shape[0] if x.ndim == 4 else 1), x.shape[-3], x.shape[-2]


def _checked_frames(frames, what, bgr=True):
    if isinstance(frames, NV12Frames):
        if not bgr:
            raise ValueError('%s: bgr=False has no meaning for NV12Frames' % what)
        if len(frames.lead) != 1:
            raise ValueError('%s takes NV12Frames of (n, H, W), got y %s' % (what, tuple(frames.y.shape)))
        return frames
    x = frames if torch.is_tensor(frames) else np.asarray(frames)
    if x.dtype != (torch.uint8 if torch.is_tensor(x) else np.uint8):
        raise ValueError('%s takes uint8 frames, got %s' % (what, x.dtype))
    if x.ndim not in (3, 4) or x.shape[-1] != 3:
        raise ValueError('frames must be (H, W, 3) or (n, H, W, 3), got %s' % (tuple(x.shape),))
    return x


def _device_plane(x, device, what):
    """One plane (n, rows, W) of an NV12Frames -> the device tensor, read in place where its rows are
    contiguous, and its (row, frame) strides in bytes."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.to(device)
    if x.device.type != 'cuda':
        raise _lib.HPEError('%s needs a ROCm GPU (MI355X / gfx950), got device %s' % (what, x.device))
    if not (x.stride(2) == 1 and x.stride(1) >= x.shape[2]):
        x = x.contiguous()
    return x, (x.stride(1), x.stride(0))


def _device_frames(x, device, out, what):
    """checked uint8 (H, W, 3) / (n, H, W, 3) frames -> (the (n, H, W, 3) device tensor, its row stride
    in bytes).  A device tensor whose pixels are contiguous is read in place through its row stride.
    Checked NV12Frames -> (the NV12Frames of the two device planes, their (y row, y frame, uv row, uv
    frame) strides in bytes)."""
    if isinstance(x, NV12Frames):
        if device is None:
            device = next((p.device for p in (x.y, x.uv) if torch.is_tensor(p) and p.is_cuda),
                          out.device if out is not None else 'cuda')
        (y, sy), (uv, suv) = _device_plane(x.y, device, what), _device_plane(x.uv, device, what)
        return NV12Frames(y, uv, x.matrix), sy + suv
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() == 3:
        x = x[None]
    if device is None:
        device = x.device if x.is_cuda else (out.device if out is not None else 'cuda')
    x = x.to(device)
    if x.device.type != 'cuda':
        raise _lib.HPEError('%s needs a ROCm GPU (MI355X / gfx950), got device %s' % (what, x.device))
    n, h, w, _ = x.shape
    sn, sh, sw, sc = x.stride()
    if not (sc == 1 and sw == 3 and sh >= 3 * w and (n <= 1 or sn == h * sh)):
        x = x.contiguous()
        sh = 3 * w
    return x, sh


def _out_tensor(out, n, oh, ow, device):
    if out is None:
        return torch.empty((n, oh, ow, 3), dtype=torch.float32, device=device)
    if (tuple(out.shape) != (n, oh, ow, 3) or out.dtype != torch.float32 or out.device != device
            or not out.is_contiguous()):
        raise ValueError('out must be a contiguous float32 (%d, %d, %d, 3) tensor on %s' % (n, oh, ow, device))
    return out


def _out_hw(size):
    """size: int or (h, w) of the network input -> (h, w)."""
    return (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))


def _launch(name, device, *args):
    """Call the library's ``name(*args, stream)`` on ``device`` and its current stream and check it."""
    fn = getattr(_lib.load(), name)
    with torch.cuda.device(device):
        _lib.check(fn(*args, _lib.stream()), name)


def _source(x, device, out, what, bgr, rois):
    """Checked frames of either kind -> (the device frames, the entry point that reads them — the ROI
    form if ``rois`` —, its arguments before the crop rectangle or the ROI table, those between that and
    ``out``): the frames' pointers, count, size and strides, and the matrix or the bgr flag where the
    entry point's signature has it."""
    x, strides = _device_frames(x, device, out, what)
    n, h, w = frame_dims(x)
    if isinstance(x, NV12Frames):
        lead, colour = (_lib.ptr(x.y), _lib.ptr(x.uv), n, h, w) + strides, (MATRICES[x.matrix],)
        return (x, 'hpe_preprocess_rois_nv12', lead, colour) if rois else (x, 'hpe_preprocess_nv12', lead + colour, ())
    return x, 'hpe_preprocess_rois' if rois else 'hpe_preprocess', (_lib.ptr(x), n, h, w, strides), (int(bool(bgr)),)


def prepare_input(frames, size=128, bgr=True, crop=None, device=None, out=None):
    """frames: uint8 (H, W, 3) or (n, H, W, 3), numpy array or tensor, host or device.  size: int or
    (h, w) of the network input (128: front model, 256: back model).  bgr: the input is BGR (cv2
    frames) and is reversed to RGB.  Returns the device tensor (n, h, w, 3) float32 (``out`` if given).
    A device tensor whose pixels are contiguous is read in place through its row stride.  An NV12Frames
    stands for the BGR frames it converts to (hpe_preprocess_nv12); bgr=False is refused with one."""
    oh, ow = _out_hw(size)
    x, name, lead, colour = _source(_checked_frames(frames, 'prepare_input', bgr), device, out, 'prepare_input', bgr,
                                    rois=False)
    n, h, w = frame_dims(x)
    out = _out_tensor(out, n, oh, ow, x.device)
    _launch(name, x.device, *lead, *crop_rect(h, w, crop), *colour, _lib.ptr(out), oh, ow)
    return out


def pad_bytes(pad_value):
    """int or 3-tuple in the frame's channel order -> three ints in 0..255."""
    p = (pad_value,) * 3 if np.isscalar(pad_value) else tuple(pad_value)
    if len(p) != 3 or any(int(v) != v or not 0 <= int(v) <= 255 for v in p):
        raise ValueError('pad_value must be an int or three ints in 0..255, got %r' % (pad_value,))
    return tuple(int(v) for v in p)


def roi_table(rois):
    """(m, 5) int array-like or int32 tensor of (frame, x0, y0, w, h) rows -> the int32 tensor, where
    it is."""
    if torch.is_tensor(rois):
        if rois.dtype != torch.int32:
            raise ValueError('a rois tensor must be int32, got %s' % (rois.dtype,))
        t = rois
    else:
        a = np.asarray(rois)
        if a.size == 0:
            a = a.reshape(-1, 5).astype(np.int32) if a.ndim < 2 else a.astype(np.int32)
        if a.dtype.kind not in 'iu':
            raise ValueError('rois must be integers, got %s' % (a.dtype,))
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError('rois must fit int32')
        t = torch.from_numpy(np.ascontiguousarray(a, np.int32))
    if t.dim() != 2 or t.shape[1] != 5:
        raise ValueError('rois must be (m, 5) rows of (frame, x0, y0, w, h), got %s' % (tuple(t.shape),))
    return t


def tile_offsets(length, tile, overlap):
    """Offsets of the tiles of side ``tile`` along an axis of ``length`` pixels, neighbours overlapping
    by at least ``overlap``: the first starts at 0, the last ends at ``length``, every pixel is covered.
    An axis no longer than the tile gets one centred tile (a negative offset: its outside is padded)."""
    if length <= tile:
        return [-((tile - length) // 2)]
    step = tile - overlap
    n = -(-(length - tile) // step) + 1
    return [(i * (length - tile)) // (n - 1) for i in range(n)]


def tile_rois(n_frames, h, w, tile, overlap, crop=None, full=True):
    """The ROI table of tiled detection for ``n_frames`` frames of h x w: per frame, the rectangle
    crop_rect(h, w, crop) that detect_images(crop=) looks at (row 0, if ``full``), then square tiles of
    side ``tile`` over that rectangle, row-major (y outer, x inner), positioned by tile_offsets along
    each axis.  tile=None: row 0 only.  Returns (rois (n_frames * R, 5) int32, R): frame-major, rows
    f*R .. f*R+R-1 are frame f's, each (f, x0, y0, w, h) — the table of prepare_rois."""
    sx, sy, sw, sh = crop_rect(h, w, crop)
    if tile is None:
        if not full:
            raise ValueError('tile_rois: full=False with tile=None leaves no rows')
        rows = []
    else:
        tile, overlap = int(tile), int(overlap)
        if tile < 1:
            raise ValueError('tile_rois: tile must be at least 1, got %d' % tile)
        if not 0 <= overlap < tile:
            raise ValueError('tile_rois: overlap must be in 0 .. tile - 1 = %d, got %d' % (tile - 1, overlap))
        rows = [(sx + ox, sy + oy, tile, tile) for oy in tile_offsets(sh, tile, overlap)
                for ox in tile_offsets(sw, tile, overlap)]
    if full:
        rows.insert(0, (sx, sy, sw, sh))
    per_frame = np.asarray(rows, np.int64).reshape(len(rows), 4)
    if np.abs(per_frame).max() >= 2 ** 31:
        raise ValueError('tile_rois: rows must fit int32')
    rois = np.empty((int(n_frames), len(rows), 5), np.int32)
    rois[:, :, 0] = np.arange(int(n_frames), dtype=np.int32)[:, None]
    rois[:, :, 1:] = per_frame.astype(np.int32)
    return rois.reshape(-1, 5), len(rows)


def prepare_rois(frames, rois, size=128, bgr=True, pad_value=0, device=None, out=None):
    """prepare_input per region of interest.  frames as prepare_input; rois: (m, 5) int array-like or
    int32 device tensor, row r = (frame, x0, y0, w, h) in frame pixels, which may reach outside the
    frame; pad_value: int or 3-tuple in the frame's channel order, the canvas outside the frame.
    Returns the device tensor (m, h, w, 3) float32 (``out`` if given): row r is prepare_input of the
    h x w canvas of ROI r.  An invalid row (frame outside 0..n-1, w or h outside 1..2^24, |x0| or |y0|
    above 2^24) gives the prepared pad value.  With an NV12Frames (hpe_preprocess_rois_nv12) the pad
    bytes are B, G, R and are used as they are, not converted."""
    x = _checked_frames(frames, 'prepare_rois', bgr)
    t = roi_table(rois)
    p0, p1, p2 = pad_bytes(pad_value)
    oh, ow = _out_hw(size)
    x, name, lead, colour = _source(x, device, out, 'prepare_rois', bgr, rois=True)
    t = t.to(x.device).contiguous()
    m = t.shape[0]
    out = _out_tensor(out, m, oh, ow, x.device)
    _launch(name, x.device, *lead, _lib.ptr(t), m, p0, p1, p2, *colour, _lib.ptr(out), oh, ow)
    return out
