"""NV12 -> BGR as include/hpe.h states it for hpe_preprocess_nv12 / hpe_preprocess_rois_nv12, restated
in numpy (int64 inside, so nothing here can overflow): the chroma of pixel (y, x) is the pair
uv[y >> 1][x >> 1], and

    yy = max(Y - 16, 0) * CY,  u = U - 128,  v = V - 128
    R = sat8((yy + CVR * v           + (1 << 19)) >> 20)
    G = sat8((yy + CVG * v + CUG * u + (1 << 19)) >> 20)
    B = sat8((yy + CUB * u           + (1 << 19)) >> 20)

with >> a floor and sat8 a clamp to 0..255.  "NV12 in" is then, by definition, the BGR path on
nv12_to_bgr(frames): tests/test_nv12.py compares the two with assert_array_equal.

OpenCV parity is unpinned (cv2 is not a dependency): 'bt601' carries the constants of OpenCV's
COLOR_YUV2BGR_NV12, 'bt709' is round(c * 2^20) of the exact BT.709 limited-range matrix."""
import numpy as np

SHIFT = 20
# matrix -> (CY, CVR, CVG, CUG, CUB)
COEF = {
    'bt601': (1220542, 1673527, -852492, -409993, 2116026),
    'bt709': (1220945, 1879825, -558796, -223607, 2215014),
}
MATRIX_ID = {'bt601': 0, 'bt709': 1}


def float_matrix(matrix):
    """The float64 matrix (cy, cvr, cvg, cug, cub) the table is the fixed-point form of."""
    if matrix == 'bt601':                          # the rounded BT.601 constants OpenCV starts from
        return 1.164, 1.596, -0.813, -0.391, 2.018
    kr, kb = 0.2126, 0.0722                        # BT.709, 8-bit limited range: Y 16..235, C 16..240
    kg = 1.0 - kr - kb
    cvr, cub = 255.0 / 224.0 * 2.0 * (1.0 - kr), 255.0 / 224.0 * 2.0 * (1.0 - kb)
    return 255.0 / 219.0, cvr, -cvr * kr / kg, -cub * kb / kg, cub


def sums(Y, U, V, matrix='bt601'):
    """The three sums before the shift, (r, g, b) as int64 arrays."""
    cy, cvr, cvg, cug, cub = COEF[matrix]
    yy = np.maximum(np.asarray(Y, np.int64) - 16, 0) * cy
    u = np.asarray(U, np.int64) - 128
    v = np.asarray(V, np.int64) - 128
    half = 1 << (SHIFT - 1)
    return yy + cvr * v + half, yy + cvg * v + cug * u + half, yy + cub * u + half


def convert(Y, U, V, matrix='bt601'):
    """Elementwise (Y, U, V) -> uint8 array (..., 3) in B, G, R order."""
    r, g, b = sums(Y, U, V, matrix)
    return np.stack([np.clip(c >> SHIFT, 0, 255) for c in (b, g, r)], -1).astype(np.uint8)


def convert_float(Y, U, V, matrix='bt601'):
    """The float64 matrix applied to the same (Y, U, V), rounded floor(x + 0.5) and clamped: int64
    (..., 3) in B, G, R order."""
    cy, cvr, cvg, cug, cub = float_matrix(matrix)
    yy = np.maximum(np.asarray(Y, np.float64) - 16.0, 0.0) * cy
    u = np.asarray(U, np.float64) - 128.0
    v = np.asarray(V, np.float64) - 128.0
    bgr = (yy + cub * u, yy + cvg * v + cug * u, yy + cvr * v)
    return np.stack([np.clip(np.floor(c + 0.5), 0, 255) for c in bgr], -1).astype(np.int64)


def planes(packed):
    """The packed (..., 3H/2, W) layout -> (y (..., H, W), uv (..., H/2, W))."""
    packed = np.asarray(packed)
    h = packed.shape[-2] // 3 * 2
    return packed[..., :h, :], packed[..., h:, :]


def nv12_to_bgr(y, uv, matrix='bt601'):
    """y uint8 (..., H, W), uv uint8 (..., H/2, W/2, 2) or (..., H/2, W) -> uint8 (..., H, W, 3) BGR."""
    y = np.asarray(y)
    h, w = y.shape[-2:]
    assert y.dtype == np.uint8 and h % 2 == 0 and w % 2 == 0
    uv = np.asarray(uv).reshape(y.shape[:-2] + (h // 2, w // 2, 2))
    assert uv.dtype == np.uint8
    rows, cols = (np.arange(h) >> 1)[:, None], (np.arange(w) >> 1)[None, :]
    return convert(y, uv[..., rows, cols, 0], uv[..., rows, cols, 1], matrix)
