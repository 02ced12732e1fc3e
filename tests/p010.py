"""Test-side P010 codec: the definitions of include/mm.h (MM_P010 /
MM_P010_FULL) in numpy, float64 throughout.

A frame is one uint16 array [H * 3 / 2][W]: H rows of luma words, then H / 2
rows of interleaved (Cb, Cr) words.  A word is 16-bit fixed point, v = word /
64 in 10-bit code units (P010 content has the low 6 bits zero; decode()
honours them).  decode() gives the RGBA frame a P010 frame IS (unclamped
BT.601, every chroma sample shared by its 2 x 2 pixels); encode() is the
output side (NV12's formulas on the saturated RGB, the 2 x 2 mean of the
unrounded chroma, codes floor(v + 0.5) clamped to 0 .. 1023, stored as
code << 6).
"""
import numpy as np


def _range(full):
    """-> luma offset, luma scale, chroma scale (10-bit code units)"""
    return (0.0, 1023.0, 1023.0) if full else (64.0, 876.0, 896.0)


def decode(buf, dtype=np.float32, full=False):
    """P010 words [H*3/2][W] -> RGBA [H][W][4] of `dtype` (alpha 1, not clamped)."""
    assert buf.dtype == np.uint16
    H = buf.shape[0] * 2 // 3
    W = buf.shape[1]
    y0, ys, cs = _range(full)
    v = buf.astype(np.float64) / 64.0
    y = (v[:H] - y0) / ys
    c = v[H:].reshape(H // 2, W // 2, 2)
    cb = np.repeat(np.repeat((c[..., 0] - 512.0) / cs, 2, axis=0), 2, axis=1)
    cr = np.repeat(np.repeat((c[..., 1] - 512.0) / cs, 2, axis=0), 2, axis=1)
    out = np.empty((H, W, 4), np.float64)
    out[..., 0] = y + 1.402 * cr
    out[..., 1] = y - 0.344136 * cb - 0.714136 * cr
    out[..., 2] = y + 1.772 * cb
    out[..., 3] = 1.0
    return out.astype(dtype)


def _words(v):
    return (np.clip(np.floor(v + 0.5), 0, 1023).astype(np.uint16) << 6).astype(np.uint16)


def encode(rgb, full=False):
    """RGB(A) [H][W][>=3] (uint8: byte / 255; float: saturated here) -> P010
    words [H*3/2][W], every one code << 6."""
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
    out = np.empty((H * 3 // 2, W), np.uint16)
    out[:H] = _words(yl * ys + y0)
    out[H:, 0::2] = _words(mean(cb) * cs + 512.0)
    out[H:, 1::2] = _words(mean(cr) * cs + 512.0)
    return out


def chroma_stress(buf, t):
    """The frame with its CbCr plane replaced by a gradient over the whole legal
    range 64 .. 960 (10-bit codes) that moves with t: Cb along x, Cr along y.
    Decodes to RGB far out of gamut (limited range): exercises the unclamped
    decode and the output saturate."""
    H = buf.shape[0] * 2 // 3
    W = buf.shape[1]
    out = buf.copy()
    x = (np.arange(W // 2) + 5 * t) % (W // 2)
    yy = (np.arange(H // 2) + 3 * t) % (H // 2)
    cb = 64 + np.round(x * (896.0 / (W // 2 - 1))).astype(np.int64)
    cr = 64 + np.round(yy * (896.0 / (H // 2 - 1))).astype(np.int64)
    out[H:, 0::2] = (cb << 6).astype(np.uint16)[None, :]
    out[H:, 1::2] = (cr << 6).astype(np.uint16)[:, None]
    return out


def from_nv12(buf_u8):
    """An NV12 frame as P010 words, u8 << 8 (the 10-bit code 4 c).  In limited
    range (4 c - 64) / 876 = (c - 16) / 219 and (4 c - 512) / 896 = (c - 128) /
    224: the P010 frame decodes to exactly the NV12 frame's RGBA."""
    assert buf_u8.dtype == np.uint8
    return (buf_u8.astype(np.uint16) << 8).astype(np.uint16)
