"""Test-side helpers for the three-plane 8-bit 4:2:0 format of include/mm.h:
MM_I420, its _FULL code and the matrix bits.

An I420 frame IS the NV12 frame with the same samples, so there is no codec
here: tests/nv12.py / tests/ycbcr.py encode and decode, and from_nv12 /
to_nv12 move the chroma bytes, a pure permutation.  A frame is one uint8 array
[H * 3 / 2][W], the frame's bytes in NV12's shape: W H luma bytes, then the
Cb plane (H/2 rows of W/2 bytes), then the Cr plane (rows of the array and
chroma rows coincide only where they happen to).

The surface helpers at the end handle the three planes under a layout, on
frames as their tight bytes (flat uint8 arrays), like tests/y210.py: the Cr
plane lies chroma_pitch x H/2 bytes after the Cb plane.
"""
import numpy as np

import ycbcr

PLANAR = 512  # MM_PLANAR
UNIT = 1      # pitches, offsets, strides and frame pointers: any byte
TAIL = 64     # bytes kept after the last frame's extent
POISON = 0xFF


def fmt_code(matrix=601, full=False):
    """The format code of include/mm.h."""
    return ycbcr.fmt_code(matrix, full) | PLANAR


def nv12_code(fmt):
    """The NV12 code with the same range and matrix."""
    return fmt & ~PLANAR


def from_nv12(buf):
    """NV12 bytes [H*3/2][W] -> I420 bytes in the same shape."""
    assert buf.dtype == np.uint8 and buf.ndim == 2 and buf.shape[0] % 3 == 0 and buf.shape[1] % 2 == 0
    H, W = buf.shape[0] * 2 // 3, buf.shape[1]
    out = np.empty(buf.size, np.uint8)
    out[:W * H] = buf[:H].reshape(-1)
    c = buf[H:].reshape(H // 2, W // 2, 2)
    out[W * H:W * H * 5 // 4] = c[..., 0].reshape(-1)
    out[W * H * 5 // 4:] = c[..., 1].reshape(-1)
    return out.reshape(buf.shape)


def to_nv12(buf):
    """I420 bytes [H*3/2][W] -> NV12 bytes in the same shape."""
    assert buf.dtype == np.uint8 and buf.ndim == 2 and buf.shape[0] % 3 == 0 and buf.shape[1] % 2 == 0
    H, W = buf.shape[0] * 2 // 3, buf.shape[1]
    p = buf.reshape(-1)
    out = np.empty((H * 3 // 2, W), np.uint8)
    out[:H] = p[:W * H].reshape(H, W)
    out[H:, 0::2] = p[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    out[H:, 1::2] = p[W * H * 5 // 4:].reshape(H // 2, W // 2)
    return out


# ---- surfaces: three planes, unit 1 ----------------------------------------------
def planes(W, H, lay):
    """(offset in the surface, pitch, rows, row bytes, offset in the tight frame) per plane."""
    cr = lay.chroma_pitch * (H // 2)
    return ((0, lay.pitch, H, W, 0),
            (lay.chroma_offset, lay.chroma_pitch, H // 2, W // 2, W * H),
            (lay.chroma_offset + cr, lay.chroma_pitch, H // 2, W // 2, W * H * 5 // 4))


def extent(W, H, lay):
    """The byte after the last Cr sample."""
    off, pitch, rows, rb, _ = planes(W, H, lay)[2]
    return off + (rows - 1) * pitch + rb


def layout(fmt, pitch, chroma_offset, chroma_pitch, frame_stride=0):
    import mm355
    return mm355.Surface(format=fmt, pitch=pitch, chroma_offset=chroma_offset, chroma_pitch=chroma_pitch,
                         frame_stride=frame_stride)


def buffer_bytes(W, H, lay, n, base=0):
    return base + (n - 1) * lay.frame_stride + extent(W, H, lay) + TAIL


def scatter(W, H, frames, lay, base=0, fill=POISON, size=None):
    """Tight frames (flat bytes) -> one pitched buffer, every other byte `fill`."""
    buf = np.full(size or buffer_bytes(W, H, lay, len(frames), base), fill, np.uint8)
    for k, f in enumerate(frames):
        f = np.asarray(f).reshape(-1)
        at = base + k * lay.frame_stride
        for off, pitch, rows, rb, src in planes(W, H, lay):
            for r in range(rows):
                buf[at + off + r * pitch: at + off + r * pitch + rb] = f[src + r * rb: src + (r + 1) * rb]
    return buf


def sample_mask(W, H, lay, n, size, base=0):
    m = np.zeros(size, bool)
    for k in range(n):
        at = base + k * lay.frame_stride
        for off, pitch, rows, rb, _ in planes(W, H, lay):
            for r in range(rows):
                m[at + off + r * pitch: at + off + r * pitch + rb] = True
    return m


def gather(W, H, buf, lay, n, base=0):
    out = []
    for k in range(n):
        at = base + k * lay.frame_stride
        f = np.empty(W * H * 3 // 2, np.uint8)
        for off, pitch, rows, rb, dst in planes(W, H, lay):
            for r in range(rows):
                f[dst + r * rb: dst + (r + 1) * rb] = buf[at + off + r * pitch: at + off + r * pitch + rb]
        out.append(f)
    return out
