"""Test-side codec for the packed 8-bit Y'CbCr 4:2:2 formats of include/mm.h:
MM_YUY2 / MM_UYVY, their _FULL codes and the matrix bits, in numpy, float64
throughout.  The definitions (ranges, matrices, decode coefficients) are those
of tests/ycbcr.py, reused here.

A frame is uint8 [H][2 W]: rows of W / 2 four-byte macropixels, bytes
Y0 Cb Y1 Cr (YUY2) or Cb Y0 Cr Y1 (UYVY).  decode() gives the RGBA frame a
frame IS (every chroma sample shared by its 1 x 2 pixels, unclamped); encode()
is the output side: of the saturated RGB, Y', Cb', Cr' by the matrix's weights,
the 1 x 2 mean of the unrounded chroma, codes floor(v + 0.5) clamped.

The surface helpers at the end handle the one-plane layout with unit 4, on
frames as their tight bytes (flat uint8 arrays), like tests/surface.py.
"""
import numpy as np

import ycbcr
from ycbcr import KRKB, _range, decode_coeffs

UNIT = 4      # one macropixel: what pitches, strides and frame pointers are multiples of
TAIL = 64     # bytes kept after the last frame's extent


def fmt_code(matrix=601, full=False, uyvy=False):
    """The format code of include/mm.h."""
    return 24 + (2 if uyvy else 0) + (1 if full else 0) + ycbcr.matrix_bit(matrix)


def _offsets(uyvy):
    """-> byte of Y0, Cb in the macropixel (Y1 and Cr two bytes further)."""
    return (1, 0) if uyvy else (0, 1)


def split(buf, uyvy=False):
    """Frame [H][2 W] -> (Y [H][W], Cb [H][W/2], Cr [H][W/2]) codes."""
    assert buf.dtype == np.uint8 and buf.ndim == 2 and buf.shape[1] % 4 == 0
    yo, co = _offsets(uyvy)
    return buf[:, yo::2], buf[:, co::4], buf[:, co + 2::4]


def join(y, cb, cr, uyvy=False):
    """(Y [H][W], Cb [H][W/2], Cr [H][W/2]) codes -> frame [H][2 W]."""
    H, W = y.shape
    yo, co = _offsets(uyvy)
    out = np.empty((H, 2 * W), np.uint8)
    out[:, yo::2] = y
    out[:, co::4] = cb
    out[:, co + 2::4] = cr
    return out


def swap_order(buf):
    """The bytes of every 16-bit pair swapped: YUY2 <-> UYVY of the same picture."""
    return np.ascontiguousarray(buf.reshape(buf.shape[0], -1, 2)[:, :, ::-1]).reshape(buf.shape)


def decode(buf, dtype=np.float32, matrix=601, full=False, uyvy=False):
    """Frame [H][2 W] uint8 -> RGBA [H][W][4] of `dtype` (alpha 1, not clamped)."""
    yc, cbc, crc = split(buf, uyvy)
    H, W = yc.shape
    y0, ys, cs, mid = _range(full, 8)
    y = (yc.astype(np.float64) - y0) / ys
    cb = np.repeat((cbc.astype(np.float64) - mid) / cs, 2, axis=1)
    cr = np.repeat((crc.astype(np.float64) - mid) / cs, 2, axis=1)
    rcr, gcb, gcr, bcb = decode_coeffs(matrix)
    out = np.empty((H, W, 4), np.float64)
    out[..., 0] = y + rcr * cr
    if matrix == 601:
        out[..., 1] = y - (-gcb) * cb - (-gcr) * cr    # ycbcr.py's order of operations
    else:
        out[..., 1] = y + gcb * cb + gcr * cr
    out[..., 2] = y + bcb * cb
    out[..., 3] = 1.0
    return out.astype(dtype)


def _codes(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def encode(rgb, matrix=601, full=False, uyvy=False):
    """RGB(A) [H][W][>=3] (uint8: byte / 255; float: saturated here) -> frame
    [H][2 W] uint8."""
    a = np.asarray(rgb)
    f = a[..., :3].astype(np.float64) / 255.0 if a.dtype == np.uint8 else a[..., :3].astype(np.float64)
    f = np.clip(f, 0.0, 1.0)
    H, W = f.shape[:2]
    assert W % 2 == 0
    y0, ys, cs, mid = _range(full, 8)
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
    mean = lambda p: p.reshape(H, W // 2, 2).mean(axis=2)
    return join(_codes(yl * ys + y0), _codes(mean(cb) * cs + mid), _codes(mean(cr) * cs + mid), uyvy)


def chroma_stress(buf, t, uyvy=False):
    """The frame with its chroma bytes replaced by a gradient over the whole
    legal range 16 .. 240 that moves with t: Cb along x, Cr along y.  Decodes
    far out of gamut under every matrix."""
    y, _, _ = split(buf, uyvy)
    H, W = y.shape
    x = (np.arange(W // 2) + 5 * t) % (W // 2)
    yy = (np.arange(H) + 3 * t) % H
    cb = 16 + np.round(x * (224.0 / (W // 2 - 1))).astype(np.int64)
    cr = 16 + np.round(yy * (224.0 / (H - 1))).astype(np.int64)
    return join(y, np.broadcast_to(cb[None, :], (H, W // 2)), np.broadcast_to(cr[:, None], (H, W // 2)), uyvy)


# ---- surfaces: one plane, unit 4 -------------------------------------------------
def row_bytes(W):
    return 2 * W


def lay_roi(fmt, W, H, PW, PH, x, y):
    """The W x H region at (x, y), x even, of a tight PW x PH parent: (layout,
    byte offset of the region's first macropixel in the parent, the parent's bytes)."""
    import mm355
    assert x % 2 == 0 and PW % 2 == 0
    s = mm355.Surface(format=fmt, pitch=2 * PW)
    s.frame_stride = 2 * PW * PH
    return s, y * 2 * PW + 2 * x, 2 * PW * PH


def buffer_bytes(W, H, lay, n, base=0):
    return base + (n - 1) * lay.frame_stride + lay.bytes(W, H) + TAIL


def scatter(W, H, frames, lay, base=0, fill=0xFF, size=None):
    """Tight frames (flat bytes) -> one pitched buffer, every other byte `fill`."""
    rb = row_bytes(W)
    buf = np.full(size or buffer_bytes(W, H, lay, len(frames), base), fill, np.uint8)
    for k, f in enumerate(frames):
        at = base + k * lay.frame_stride
        for r in range(H):
            buf[at + r * lay.pitch: at + r * lay.pitch + rb] = f[r * rb:(r + 1) * rb]
    return buf


def sample_mask(W, H, lay, n, size, base=0):
    rb = row_bytes(W)
    m = np.zeros(size, bool)
    for k in range(n):
        at = base + k * lay.frame_stride
        for r in range(H):
            m[at + r * lay.pitch: at + r * lay.pitch + rb] = True
    return m


def gather(W, H, buf, lay, n, base=0):
    rb = row_bytes(W)
    out = []
    for k in range(n):
        at = base + k * lay.frame_stride
        f = np.empty(rb * H, np.uint8)
        for r in range(H):
            f[r * rb:(r + 1) * rb] = buf[at + r * lay.pitch: at + r * lay.pitch + rb]
        out.append(f)
    return out
