"""Test-side codec of the single-plane grayscale formats: the definitions of
include/mm.h (MM_Y8 / MM_Y10 / MM_Y12 / MM_Y16) in numpy, float64 throughout,
plus the synthetic gray clips and the pitched-buffer helpers their tests share.

A frame is one array [H][W] of uint8 (8 bits) or uint16 (10, 12, 16 bits, the
code in the LOW bits).  decode() gives the RGBA frame such a frame IS
(R = G = B = sample / max, alpha 1, not clamped: a word above max decodes above
1); encode() is the output side (Yl = 0.299 R + 0.587 G + 0.114 B of the
saturated RGB, code floor(Yl max + 0.5) clamped to 0 .. max).
"""
import functools

import numpy as np

BITS = (8, 10, 12, 16)


def vmax(bits):
    assert bits in BITS, bits
    return (1 << bits) - 1


def dtype_of(bits):
    return np.uint8 if bits == 8 else np.uint16


def fmt_of(bits):
    import mm355
    return {8: mm355.Y8, 10: mm355.Y10, 12: mm355.Y12, 16: mm355.Y16}[bits]


def decode(buf, bits, dtype=np.float32):
    """samples [H][W] -> RGBA [H][W][4] of `dtype` (alpha 1, not clamped)."""
    v = np.asarray(buf).astype(np.float64) / float(vmax(bits))
    out = np.empty(v.shape + (4,), np.float64)
    out[..., 0] = out[..., 1] = out[..., 2] = v
    out[..., 3] = 1.0
    return out.astype(dtype)


def codes(v, bits):
    """values (saturated here) -> codes floor(v max + 0.5) clamped to 0 .. max."""
    m = float(vmax(bits))
    v = np.clip(np.asarray(v).astype(np.float64), 0.0, 1.0)
    return np.clip(np.floor(v * m + 0.5), 0, m).astype(dtype_of(bits))


def encode(rgb, bits):
    """RGB(A) [H][W][>=3] float (saturated here) -> samples [H][W]."""
    f = np.clip(np.asarray(rgb)[..., :3].astype(np.float64), 0.0, 1.0)
    return codes(0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2], bits)


# ---- synthetic gray clips ------------------------------------------------------
def _scene(W, H, t):
    """A float64 picture in about 0.1 .. 0.85 that moves by +-0.5 pixel (the
    stream of SURVEY.md 8d, one channel, before any quantising)."""
    rng = np.random.default_rng(0x5EED)
    noise = rng.random((H, W))          # fixed per pixel, as the synthetic stream's
    x = np.arange(W)[None, :].astype(np.float64)
    y = np.arange(H)[:, None].astype(np.float64)
    d = 0.5 * np.sin(2.0 * np.pi * 0.05 * t)
    return 0.4 + 0.3 * np.sin(2.0 * np.pi * (x + d) / 37.0) * np.cos(2.0 * np.pi * y / 53.0) + 0.15 * noise


@functools.lru_cache(maxsize=None)
def frames(W, H, n, bits, stretch=False, stray=False, dim=1.0):
    """n frames of the clip quantised to `bits` (read-only arrays).  stretch:
    stretched about mid-gray by a gain of 3 before quantising (a third of the
    picture then sits at code 0 or max: the saturate stress).  stray (10 and 12
    bits): a few words of every frame carry bits above the code.  dim: the
    picture times this factor (an underexposed camera)."""
    out = []
    rng = np.random.default_rng(bits)
    for t in range(n):
        v = _scene(W, H, t) * dim
        if stretch:
            v = 0.5 + 3.0 * (v - 0.5)
        buf = codes(v, bits)
        if stray:
            assert bits in (10, 12)
            at = rng.integers(0, buf.size, 16)
            buf.reshape(-1)[at] |= np.uint16(0x8000 | (1 << bits))
        buf.setflags(write=False)
        out.append(buf)
    return tuple(out)


def as_bytes(f):
    """[H][W] samples -> [H][W * sample bytes] uint8 (how the tests move words:
    nothing depends on a 16-bit tensor type)."""
    return np.ascontiguousarray(f).view(np.uint8)


def from_bytes(b, bits):
    return np.ascontiguousarray(b).view(dtype_of(bits))


# ---- pitched buffers -----------------------------------------------------------
POISON = 0xFF


def scatter(fr, pitch, stride, size):
    """Tight frames [H][W] -> one pitched uint8 buffer, every other byte POISON."""
    buf = np.full(size, POISON, np.uint8)
    for k, f in enumerate(fr):
        b = as_bytes(f)
        for r in range(b.shape[0]):
            at = k * stride + r * pitch
            buf[at:at + b.shape[1]] = b[r]
    return buf


def sample_mask(H, row_bytes, n, pitch, stride, size):
    m = np.zeros(size, bool)
    for k in range(n):
        for r in range(H):
            at = k * stride + r * pitch
            m[at:at + row_bytes] = True
    return m


def gather(buf, H, row_bytes, n, pitch, stride, bits):
    out = []
    for k in range(n):
        rows = [buf[k * stride + r * pitch: k * stride + r * pitch + row_bytes] for r in range(H)]
        out.append(from_bytes(np.stack(rows), bits))
    return out


def sentinel(size):
    return ((np.arange(size, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
