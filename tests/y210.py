"""Test-side codec for the 10-bit packed Y'CbCr 4:2:2 format of include/mm.h:
MM_Y210, its _FULL code and the matrix bits, in numpy, float64 throughout.
The definitions (ranges, matrices, decode coefficients) are those of
tests/ycbcr.py at depth 10, reused here.

A frame is uint16 [H][2 W]: rows of W / 2 eight-byte macropixels, words
Y0 Cb Y1 Cr, each read as 16-bit fixed point, v = word / 64 in 10-bit code
units (Y210 content has the low 6 bits zero; Y216's are honoured).  decode()
gives the RGBA frame a frame IS (every chroma sample shared by its 1 x 2 pixels,
unclamped); encode() is the output side: of the saturated RGB, Y', Cb', Cr' by
the matrix's weights, the 1 x 2 mean of the unrounded chroma, codes
floor(v + 0.5) clamped to 0 .. 1023 and stored << 6.

The surface helpers at the end handle the one-plane layout with unit 8, on
frames as their tight bytes (flat uint8 arrays), like tests/yuv422.py.
"""
import numpy as np

import ycbcr
from ycbcr import KRKB, _range, decode_coeffs

UNIT = 8      # one macropixel: what pitches, strides and frame pointers are multiples of
TAIL = 64     # bytes kept after the last frame's extent


def fmt_code(matrix=601, full=False):
    """The format code of include/mm.h."""
    return 22 + (1 if full else 0) + ycbcr.matrix_bit(matrix)


def split(buf):
    """Frame [H][2 W] -> (Y [H][W], Cb [H][W/2], Cr [H][W/2]) words."""
    assert buf.dtype == np.uint16 and buf.ndim == 2 and buf.shape[1] % 4 == 0
    return buf[:, 0::2], buf[:, 1::4], buf[:, 3::4]


def join(y, cb, cr):
    """(Y [H][W], Cb [H][W/2], Cr [H][W/2]) words -> frame [H][2 W]."""
    H, W = y.shape
    out = np.empty((H, 2 * W), np.uint16)
    out[:, 0::2] = y
    out[:, 1::4] = cb
    out[:, 3::4] = cr
    return out


def from_yuy2(buf):
    """A YUY2 frame (uint8 [H][2 W]) as Y210: every byte in its word's high byte."""
    assert buf.dtype == np.uint8
    return (buf.astype(np.uint16) << 8).astype(np.uint16)


def decode(buf, dtype=np.float32, matrix=601, full=False):
    """Frame [H][2 W] uint16 -> RGBA [H][W][4] of `dtype` (alpha 1, not clamped)."""
    yw, cbw, crw = split(buf)
    H, W = yw.shape
    y0, ys, cs, mid = _range(full, 10)
    y = (yw.astype(np.float64) / 64.0 - y0) / ys
    cb = np.repeat((cbw.astype(np.float64) / 64.0 - mid) / cs, 2, axis=1)
    cr = np.repeat((crw.astype(np.float64) / 64.0 - mid) / cs, 2, axis=1)
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
    return (np.clip(np.floor(v + 0.5), 0, 1023).astype(np.uint16) << 6).astype(np.uint16)


def encode(rgb, matrix=601, full=False):
    """RGB(A) [H][W][>=3] (uint8: byte / 255; float: saturated here) -> frame
    [H][2 W] uint16, codes << 6."""
    a = np.asarray(rgb)
    f = a[..., :3].astype(np.float64) / 255.0 if a.dtype == np.uint8 else a[..., :3].astype(np.float64)
    f = np.clip(f, 0.0, 1.0)
    H, W = f.shape[:2]
    assert W % 2 == 0
    y0, ys, cs, mid = _range(full, 10)
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
    return join(_codes(yl * ys + y0), _codes(mean(cb) * cs + mid), _codes(mean(cr) * cs + mid))


def chroma_stress(buf, t):
    """The frame with its chroma words replaced by a gradient over the whole
    legal range 64 .. 960 (codes, stored << 6) that moves with t: Cb along x, Cr
    along y.  Decodes far out of gamut under every matrix."""
    y, _, _ = split(buf)
    H, W = y.shape
    x = (np.arange(W // 2) + 5 * t) % (W // 2)
    yy = (np.arange(H) + 3 * t) % H
    cb = (64 + np.round(x * (896.0 / (W // 2 - 1))).astype(np.int64)) << 6
    cr = (64 + np.round(yy * (896.0 / (H - 1))).astype(np.int64)) << 6
    return join(y, np.broadcast_to(cb[None, :], (H, W // 2)), np.broadcast_to(cr[:, None], (H, W // 2)))


def low_bits(buf, rng):
    """The frame with the generator's low 6 bits OR-ed into every word (Y216 content)."""
    return buf | rng.integers(0, 64, buf.shape).astype(np.uint16)


# ---- surfaces: one plane, unit 8 -------------------------------------------------
def row_bytes(W):
    return 4 * W


def lay_roi(fmt, W, H, PW, PH, x, y):
    """The W x H region at (x, y), x even, of a tight PW x PH parent: (layout,
    byte offset of the region's first macropixel in the parent, the parent's bytes)."""
    import mm355
    assert x % 2 == 0 and PW % 2 == 0
    s = mm355.Surface(format=fmt, pitch=4 * PW)
    s.frame_stride = 4 * PW * PH
    return s, y * 4 * PW + 4 * x, 4 * PW * PH


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
