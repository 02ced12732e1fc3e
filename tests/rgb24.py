"""Test-side helpers of the packed RGB formats (MM_RGB24 / MM_BGR24, include/mm.h):
the synthetic clips, the byte-order swizzle, the RGBA8 twin of a frame and the
pitched-buffer helpers their tests share.

A frame is one array [H][W][3] of uint8, bytes R G B (RGB24) or B G R (BGR24).
It IS the MM_RGBA8 frame with the same colour bytes and alpha 255: twin() makes
that frame, colour() takes the three colour bytes of an RGBA8 result back.
"""
import functools

import numpy as np

import oracle_py as O


def fmt_of(order):
    import mm355
    return {"rgb": mm355.RGB24, "bgr": mm355.BGR24}[order]


def swap(f):
    """R G B <-> B G R, a contiguous copy."""
    return np.ascontiguousarray(np.asarray(f)[..., ::-1])


def in_order(f, order):
    """A frame kept in R G B order, as `order` stores it (a writable copy)."""
    return swap(f) if order == "bgr" else np.array(f, dtype=np.uint8, order="C")


def twin(f):
    """The MM_RGBA8 frame an R G B frame IS: the same colour bytes, alpha 255."""
    f = np.asarray(f)
    out = np.full(f.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = f
    return out


def colour(rgba):
    return np.ascontiguousarray(np.asarray(rgba)[..., :3])


@functools.lru_cache(maxsize=None)
def frames(W, H, n, stretch=False):
    """n R G B frames of the project's synthetic stream (mmtest.synth's u8 frames
    without their alpha, which is 255 everywhere), read-only.  stretch: every
    byte stretched about 128 by a gain of 3, clip(floor(128 + 3 (v - 128) +
    0.5)): the saturate stress."""
    out = []
    for t in range(n):
        f = O.synth_frame(W, H, t)
        assert f.dtype == np.uint8 and f.shape == (H, W, 4) and int(f[..., 3].min()) == 255
        f = colour(f)
        if stretch:
            v = np.floor(128.0 + 3.0 * (f.astype(np.float64) - 128.0) + 0.5)
            f = np.clip(v, 0, 255).astype(np.uint8)
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


def encode(rgb):
    """float RGB(A) [H][W][>=3] -> bytes round(saturate(v) 255), MM_RGBA8's rule."""
    v = np.clip(np.asarray(rgb)[..., :3].astype(np.float64), 0.0, 1.0)
    return np.floor(v * 255.0 + 0.5).astype(np.uint8)


# ---- pitched buffers -----------------------------------------------------------
POISON = 0xFF


def scatter(fr, pitch, stride, size, base=0):
    """Tight frames [H][W][3] -> one pitched uint8 buffer (frame k at base +
    k stride, row r pitch further), every other byte POISON."""
    buf = np.full(size, POISON, np.uint8)
    for k, f in enumerate(fr):
        b = np.ascontiguousarray(f).reshape(f.shape[0], -1)
        for r in range(b.shape[0]):
            at = base + k * stride + r * pitch
            buf[at:at + b.shape[1]] = b[r]
    return buf


def sample_mask(W, H, n, pitch, stride, size, base=0):
    m = np.zeros(size, bool)
    for k in range(n):
        for r in range(H):
            at = base + k * stride + r * pitch
            m[at:at + 3 * W] = True
    return m


def gather(buf, W, H, n, pitch, stride, base=0):
    out = []
    for k in range(n):
        rows = [buf[base + k * stride + r * pitch: base + k * stride + r * pitch + 3 * W] for r in range(H)]
        out.append(np.stack(rows).reshape(H, W, 3))
    return out


def sentinel(size):
    return ((np.arange(size, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
