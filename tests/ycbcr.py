"""Test-side Y'CbCr 4:2:0 codec for every (matrix, range, depth) of
include/mm.h: MM_NV12 / MM_P010, their _FULL codes, and the matrix bits
MM_MATRIX_BT709 / MM_MATRIX_BT2020, in numpy, float64 throughout.

Frames are those of tests/nv12.py (depth 8: uint8 [H * 3 / 2][W]) and
tests/p010.py (depth 10: uint16 words, code << 6).  decode() gives the RGBA
frame a frame IS: y, cb, cr from the codes by the range's scales, then
  R = y + 2 (1 - Kr) cr,  B = y + 2 (1 - Kb) cb,
  G = y - (2 Kb (1 - Kb) / Kg) cb - (2 Kr (1 - Kr) / Kg) cr,   Kg = 1 - Kr - Kb,
unclamped, every chroma sample shared by its 2 x 2 pixels.  encode() is the
output side: of the saturated RGB, Y' = Kr R + Kg G + Kb B, Cb' = (B - Y') /
(2 (1 - Kb)), Cr' = (R - Y') / (2 (1 - Kr)), the 2 x 2 mean of the unrounded
chroma, codes floor(v + 0.5) clamped.

Matrix 601 keeps the project's standing definition, the six-digit decode
coefficients and the literal weights of nv12.py / p010.py, and reproduces those
helpers bytewise (tests/test_matrix_host.py asserts it).
"""
import numpy as np

MATRICES = (601, 709, 2020)
KRKB = {601: (0.299, 0.114), 709: (0.2126, 0.0722), 2020: (0.2627, 0.0593)}
YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])   # RGBToYIQ


def matrix_bit(matrix):
    """The MM_MATRIX_* bit of a matrix (0 for BT.601)."""
    return {601: 0, 709: 32, 2020: 64}[matrix]


def fmt_code(matrix, full=False, depth=8):
    """The format code of include/mm.h."""
    return (16 if depth == 8 else 18) + (1 if full else 0) + matrix_bit(matrix)


def _range(full, depth):
    """-> luma offset, luma scale, chroma scale, chroma midpoint (code units of `depth`)"""
    if depth == 8:
        return (0.0, 255.0, 255.0, 128.0) if full else (16.0, 219.0, 224.0, 128.0)
    return (0.0, 1023.0, 1023.0, 512.0) if full else (64.0, 876.0, 896.0, 512.0)


def decode_coeffs(matrix):
    """-> (R_cr, G_cb, G_cr, B_cb) of the decode."""
    if matrix == 601:
        return 1.402, -0.344136, -0.714136, 1.772
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    return 2.0 * (1.0 - kr), -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg, 2.0 * (1.0 - kb)


def matrix_yiq(matrix):
    """(cb, cr) -> (Y, I, Q): RGBToYIQ's rows times the decode, float64:
    [[Y_cb, Y_cr], [I_cb, I_cr], [Q_cb, Q_cr]].  BT.601's Y row is zero by
    definition (its luma weights are RGBToYIQ's own)."""
    rcr, gcb, gcr, bcb = decode_coeffs(matrix)
    m = YIQ @ np.array([[0.0, rcr], [gcb, gcr], [bcb, 0.0]])   # columns cb, cr
    if matrix == 601:
        m[0] = 0.0
    return m


def decode(buf, dtype=np.float32, matrix=601, full=False, depth=8):
    """Frame [H*3/2][W] (uint8, or uint16 words for depth 10) -> RGBA [H][W][4]
    of `dtype` (alpha 1, not clamped)."""
    assert buf.dtype == (np.uint8 if depth == 8 else np.uint16)
    H = buf.shape[0] * 2 // 3
    W = buf.shape[1]
    y0, ys, cs, mid = _range(full, depth)
    v = buf.astype(np.float64) if depth == 8 else buf.astype(np.float64) / 64.0
    y = (v[:H] - y0) / ys
    c = v[H:].reshape(H // 2, W // 2, 2)
    cb = np.repeat(np.repeat((c[..., 0] - mid) / cs, 2, axis=0), 2, axis=1)
    cr = np.repeat(np.repeat((c[..., 1] - mid) / cs, 2, axis=0), 2, axis=1)
    rcr, gcb, gcr, bcb = decode_coeffs(matrix)
    out = np.empty((H, W, 4), np.float64)
    out[..., 0] = y + rcr * cr
    if matrix == 601:
        out[..., 1] = y - (-gcb) * cb - (-gcr) * cr    # nv12.py's order of operations
    else:
        out[..., 1] = y + gcb * cb + gcr * cr
    out[..., 2] = y + bcb * cb
    out[..., 3] = 1.0
    return out.astype(dtype)


def _codes(v, depth):
    if depth == 8:
        return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    return (np.clip(np.floor(v + 0.5), 0, 1023).astype(np.uint16) << 6).astype(np.uint16)


def encode(rgb, matrix=601, full=False, depth=8):
    """RGB(A) [H][W][>=3] (uint8: byte / 255; float: saturated here) -> frame
    [H*3/2][W] (uint8, or uint16 words code << 6 for depth 10)."""
    a = np.asarray(rgb)
    f = a[..., :3].astype(np.float64) / 255.0 if a.dtype == np.uint8 else a[..., :3].astype(np.float64)
    f = np.clip(f, 0.0, 1.0)
    H, W = f.shape[:2]
    assert H % 2 == 0 and W % 2 == 0
    y0, ys, cs, mid = _range(full, depth)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    if matrix == 601:
        yl = 0.299 * r + 0.587 * g + 0.114 * b
        cb = (b - yl) * (0.5 / 0.886)
        cr = (r - yl) * (0.5 / 0.701)
    else:
        kr, kb = KRKB[matrix]
        yl = kr * r + (1.0 - kr - kb) * g + kb * b
        cb = (b - yl) * (0.5 / (1.0 - kb))
        cr = (r - yl) * (0.5 / (1.0 - kr))
    mean = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
    out = np.empty((H * 3 // 2, W), np.uint8 if depth == 8 else np.uint16)
    out[:H] = _codes(yl * ys + y0, depth)
    out[H:, 0::2] = _codes(mean(cb) * cs + mid, depth)
    out[H:, 1::2] = _codes(mean(cr) * cs + mid, depth)
    return out


def chroma_stress(buf, t, depth=8):
    """The frame with its CbCr plane replaced by a gradient over the whole legal
    range (16 .. 240, 10-bit: 64 .. 960) that moves with t: Cb along x, Cr
    along y.  Decodes far out of gamut under every matrix: exercises the
    unclamped decode, the output saturate and, for BT.709 / BT.2020, the chroma
    term of the transform's luma."""
    assert buf.dtype == (np.uint8 if depth == 8 else np.uint16)
    H = buf.shape[0] * 2 // 3
    W = buf.shape[1]
    out = buf.copy()
    lo, span, sh = (16, 224.0, 0) if depth == 8 else (64, 896.0, 6)
    x = (np.arange(W // 2) + 5 * t) % (W // 2)
    yy = (np.arange(H // 2) + 3 * t) % (H // 2)
    cb = lo + np.round(x * (span / (W // 2 - 1))).astype(np.int64)
    cr = lo + np.round(yy * (span / (H // 2 - 1))).astype(np.int64)
    out[H:, 0::2] = (cb << sh).astype(buf.dtype)[None, :]
    out[H:, 1::2] = (cr << sh).astype(buf.dtype)[:, None]
    return out
