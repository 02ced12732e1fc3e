"""Test-side NV12 codec: the definitions of include/mm.h (MM_NV12 /
MM_NV12_FULL) in numpy, float64 throughout.

A frame is one uint8 array [H * 3 / 2][W]: H rows of luma, then H / 2 rows of
interleaved (Cb, Cr) pairs.  decode() gives the RGBA frame an NV12 frame IS
(unclamped BT.601, every chroma sample shared by its 2 x 2 pixels); encode()
is the output side (y4m_from_rgba's formulas on the saturated RGB, the 2 x 2
mean of the unrounded chroma, codes floor(v + 0.5) clamped to 0 .. 255).
"""
import numpy as np


def _range(full):
    """-> luma offset, luma scale, chroma scale"""
    return (0.0, 255.0, 255.0) if full else (16.0, 219.0, 224.0)


def decode(buf, dtype=np.float32, full=False):
    """NV12 bytes [H*3/2][W] -> RGBA [H][W][4] of `dtype` (alpha 1, not clamped)."""
    H = buf.shape[0] * 2 // 3
    W = buf.shape[1]
    y0, ys, cs = _range(full)
    y = (buf[:H].astype(np.float64) - y0) / ys
    c = buf[H:].reshape(H // 2, W // 2, 2).astype(np.float64)
    cb = np.repeat(np.repeat((c[..., 0] - 128.0) / cs, 2, axis=0), 2, axis=1)
    cr = np.repeat(np.repeat((c[..., 1] - 128.0) / cs, 2, axis=0), 2, axis=1)
    out = np.empty((H, W, 4), np.float64)
    out[..., 0] = y + 1.402 * cr
    out[..., 1] = y - 0.344136 * cb - 0.714136 * cr
    out[..., 2] = y + 1.772 * cb
    out[..., 3] = 1.0
    return out.astype(dtype)


def _codes(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def encode(rgb, full=False):
    """RGB(A) [H][W][>=3] (uint8: byte / 255; float: saturated here) -> NV12
    bytes [H*3/2][W]."""
    a = np.asarray(rgb)
    f = a[..., :3].astype(np.float64) / 255.0 if a.dtype == np.uint8 else a[..., :3].astype(np.float64)
    f = np.clip(f, 0.0, 1.0)
    H, W = f.shape[:2]
    assert H % 2 == 0 and W % 2 == 0
    y0, ys, cs = _range(full)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    yl = 0.299 * r + 0.587 * g + 0.114 * b
    cb = (b - yl) * (0.5 / 0.886)
    cr = (r - yl) * (0.5 / 0.701)
    mean = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
    out = np.empty((H * 3 // 2, W), np.uint8)
    out[:H] = _codes(yl * ys + y0)
    out[H:, 0::2] = _codes(mean(cb) * cs + 128.0)
    out[H:, 1::2] = _codes(mean(cr) * cs + 128.0)
    return out


def chroma_stress(buf, t):
    """The frame with its CbCr plane replaced by a gradient over the whole legal
    range 16 .. 240 that moves with t: Cb along x, Cr along y.  Decodes to RGB
    in about -0.71 .. 1.67 (limited range): exercises the unclamped decode and
    the output saturate."""
    H = buf.shape[0] * 2 // 3
    W = buf.shape[1]
    out = buf.copy()
    x = (np.arange(W // 2) + 5 * t) % (W // 2)
    yy = (np.arange(H // 2) + 3 * t) % (H // 2)
    cb = 16 + np.round(x * (224.0 / (W // 2 - 1))).astype(np.int64)
    cr = 16 + np.round(yy * (224.0 / (H // 2 - 1))).astype(np.int64)
    out[H:, 0::2] = cb[None, :]
    out[H:, 1::2] = cr[:, None]
    return out


def matrix_iq():
    """(cb, cr) -> (I, Q): RGBToYIQ's I and Q rows times the BT.601 conversion,
    float64: [[I_cb, I_cr], [Q_cb, Q_cr]]."""
    yiq = np.array([[0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
    rgb = np.array([[0.0, 1.402], [-0.344136, -0.714136], [1.772, 0.0]])   # columns cb, cr
    return yiq @ rgb
