"""Raw camera frames -> network input on the GPU: ``prepareInputForInference`` of
BlazePoser/blazeFaceDetectorH5.py:247-269 (cv2.COLOR_BGR2RGB, / 255.0, tf.image.resize(method=
'bicubic'), (x - 0.5) / 0.5) for a batch of uint8 frames in one kernel (csrc/hpe_preproc.hip, C ABI
``hpe_preprocess``).  The frames are uploaded as bytes; everything after the upload stays on the
device.  Image decoding, webcam capture and drawing stay out of scope.
"""
import ctypes

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


def prepare_input(frames, size=128, bgr=True, crop=None, device=None, out=None):
    """frames: uint8 (H, W, 3) or (n, H, W, 3), numpy array or tensor, host or device.  size: int or
    (h, w) of the network input (128: front model, 256: back model).  bgr: the input is BGR (cv2
    frames) and is reversed to RGB.  Returns the device tensor (n, h, w, 3) float32 (``out`` if given).
    A device tensor whose pixels are contiguous is read in place through its row stride."""
    x = frames if torch.is_tensor(frames) else np.asarray(frames)
    if x.dtype != (torch.uint8 if torch.is_tensor(x) else np.uint8):
        raise ValueError('prepare_input takes uint8 frames, got %s' % (x.dtype,))
    if x.ndim not in (3, 4) or x.shape[-1] != 3:
        raise ValueError('frames must be (H, W, 3) or (n, H, W, 3), got %s' % (tuple(x.shape),))
    oh, ow = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() == 3:
        x = x[None]
    if device is None:
        device = x.device if x.is_cuda else (out.device if out is not None else 'cuda')
    x = x.to(device)
    if x.device.type != 'cuda':
        raise _lib.HPEError('prepare_input needs a ROCm GPU (MI355X / gfx950), got device %s' % (x.device,))
    n, h, w, _ = x.shape
    sn, sh, sw, sc = x.stride()
    if not (sc == 1 and sw == 3 and sh >= 3 * w and (n <= 1 or sn == h * sh)):
        x = x.contiguous()
        sh = 3 * w
    x0, y0, cw, ch = crop_rect(h, w, crop)
    if out is None:
        out = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=x.device)
    elif (tuple(out.shape) != (n, oh, ow, 3) or out.dtype != torch.float32 or out.device != x.device
          or not out.is_contiguous()):
        raise ValueError('out must be a contiguous float32 (%d, %d, %d, 3) tensor on %s' % (n, oh, ow, x.device))
    lib = _lib.load()
    with torch.cuda.device(x.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.hpe_preprocess(ctypes.c_void_p(x.data_ptr()), n, h, w, sh, x0, y0, cw, ch, int(bool(bgr)),
                                      ctypes.c_void_p(out.data_ptr()), oh, ow, stream), 'hpe_preprocess')
    return out
