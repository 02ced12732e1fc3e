"""Test-side helpers for the 10-bit three-plane 4:2:0 format of include/mm.h:
MM_I010, its _FULL code and the matrix bits (ffmpeg's yuv420p10le).

An I010 frame IS the P010 frame with the same codes: the code sits in the
word's low 10 bits instead of its high 10, and Cb and Cr lie in planes of their
own.  from_p010 / to_p010 shift by 6 and move the chroma words, nothing else.
A frame is one uint16 array [H * 3 / 2][W], the frame's words in P010's shape:
W H luma words, then the Cb plane (H/2 rows of W/2 words), then the Cr plane
(rows of the array and chroma rows coincide only where they happen to).

decode / encode are tests/ycbcr.py's depth-10 codec (float64) around that
permutation; decode does not mask the word: a word above 1023 is that value.

The surface helpers at the end handle the three planes under a layout, on
frames as their tight words (flat uint16 arrays) and buffers of words: every
offset, pitch and stride of a layout is a multiple of 2 bytes, so a pitched
buffer is a uint16 array too and `base` counts bytes (even).
"""
import numpy as np

import ycbcr

PLANAR = 512     # MM_PLANAR
LOW_BITS = 1024  # MM_LOW_BITS
UNIT = 2         # pitches, offsets, strides and frame pointers: whole words
TAIL = 64        # bytes kept after the last frame's extent
POISON = 0xFFFF


def fmt_code(matrix=601, full=False):
    """The format code of include/mm.h."""
    return ycbcr.fmt_code(matrix, full, depth=10) | PLANAR | LOW_BITS


def p010_code(fmt):
    """The P010 code with the same range and matrix."""
    return fmt & ~(PLANAR | LOW_BITS)


def from_p010(buf):
    """P010 words [H*3/2][W] (code << 6) -> I010 words in the same shape."""
    assert buf.dtype == np.uint16 and buf.ndim == 2 and buf.shape[0] % 3 == 0 and buf.shape[1] % 2 == 0
    H, W = buf.shape[0] * 2 // 3, buf.shape[1]
    s = buf >> 6
    out = np.empty(buf.size, np.uint16)
    out[:W * H] = s[:H].reshape(-1)
    c = s[H:].reshape(H // 2, W // 2, 2)
    out[W * H:W * H * 5 // 4] = c[..., 0].reshape(-1)
    out[W * H * 5 // 4:] = c[..., 1].reshape(-1)
    return out.reshape(buf.shape)


def to_p010(buf):
    """I010 words [H*3/2][W] (all <= 1023) -> P010 words in the same shape."""
    assert buf.dtype == np.uint16 and buf.ndim == 2 and buf.shape[0] % 3 == 0 and buf.shape[1] % 2 == 0
    assert int(buf.max()) <= 1023
    H, W = buf.shape[0] * 2 // 3, buf.shape[1]
    p = buf.reshape(-1)
    out = np.empty((H * 3 // 2, W), np.uint16)
    out[:H] = p[:W * H].reshape(H, W)
    out[H:, 0::2] = p[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    out[H:, 1::2] = p[W * H * 5 // 4:].reshape(H // 2, W // 2)
    return (out << 6).astype(np.uint16)


def _interleave(buf):
    """I010 words -> the same words in P010's plane shape, unshifted and unmasked (int64)."""
    H, W = buf.shape[0] * 2 // 3, buf.shape[1]
    p = buf.reshape(-1).astype(np.int64)
    out = np.empty((H * 3 // 2, W), np.int64)
    out[:H] = p[:W * H].reshape(H, W)
    out[H:, 0::2] = p[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    out[H:, 1::2] = p[W * H * 5 // 4:].reshape(H // 2, W // 2)
    return out


def decode(buf, dtype=np.float32, matrix=601, full=False):
    """I010 frame -> RGBA [H][W][4] of `dtype` (alpha 1, not clamped): v = word,
    in 10-bit code units, neither masked nor clamped; from there ycbcr.decode's
    arithmetic (float64)."""
    assert buf.dtype == np.uint16
    H, W = buf.shape[0] * 2 // 3, buf.shape[1]
    y0, ys, cs, mid = ycbcr._range(full, 10)
    v = _interleave(buf).astype(np.float64)
    y = (v[:H] - y0) / ys
    c = v[H:].reshape(H // 2, W // 2, 2)
    cb = np.repeat(np.repeat((c[..., 0] - mid) / cs, 2, axis=0), 2, axis=1)
    cr = np.repeat(np.repeat((c[..., 1] - mid) / cs, 2, axis=0), 2, axis=1)
    rcr, gcb, gcr, bcb = ycbcr.decode_coeffs(matrix)
    out = np.empty((H, W, 4), np.float64)
    out[..., 0] = y + rcr * cr
    if matrix == 601:
        out[..., 1] = y - (-gcb) * cb - (-gcr) * cr    # ycbcr.decode's order of operations
    else:
        out[..., 1] = y + gcb * cb + gcr * cr
    out[..., 2] = y + bcb * cb
    out[..., 3] = 1.0
    return out.astype(dtype)


def encode(rgb, matrix=601, full=False):
    """RGB(A) -> I010 frame: ycbcr.encode at depth 10, shifted and de-interleaved."""
    return from_p010(ycbcr.encode(rgb, matrix, full, depth=10))


# ---- surfaces: three planes of words, unit 2 ---------------------------------------
def planes(W, H, lay):
    """(byte offset in the surface, pitch in bytes, rows, row WORDS, word offset in the tight frame) per plane."""
    cr = lay.chroma_pitch * (H // 2)
    return ((0, lay.pitch, H, W, 0),
            (lay.chroma_offset, lay.chroma_pitch, H // 2, W // 2, W * H),
            (lay.chroma_offset + cr, lay.chroma_pitch, H // 2, W // 2, W * H * 5 // 4))


def extent(W, H, lay):
    """The byte after the last Cr sample."""
    off, pitch, rows, rw, _ = planes(W, H, lay)[2]
    return off + (rows - 1) * pitch + 2 * rw


def layout(fmt, pitch, chroma_offset, chroma_pitch, frame_stride=0):
    import mm355
    return mm355.Surface(format=fmt, pitch=pitch, chroma_offset=chroma_offset, chroma_pitch=chroma_pitch,
                         frame_stride=frame_stride)


def buffer_bytes(W, H, lay, n, base=0):
    return base + (n - 1) * lay.frame_stride + extent(W, H, lay) + TAIL


def _rows(W, H, lay, n, base):
    """(word index in the buffer, row words, frame, word offset in the tight frame) of every sample row."""
    assert base % 2 == 0 and lay.frame_stride % 2 == 0
    for k in range(n):
        at = base + k * lay.frame_stride
        for off, pitch, rows, rw, src in planes(W, H, lay):
            assert off % 2 == 0 and pitch % 2 == 0
            for r in range(rows):
                yield (at + off + r * pitch) // 2, rw, k, src + r * rw


def scatter(W, H, frames, lay, base=0, fill=POISON, size=None):
    """Tight frames (flat words) -> one pitched buffer of words, every other word `fill`.
    size, base: bytes."""
    nbytes = size or buffer_bytes(W, H, lay, len(frames), base)
    assert nbytes % 2 == 0
    buf = np.full(nbytes // 2, fill, np.uint16)
    fr = [np.asarray(f).reshape(-1) for f in frames]
    for at, rw, k, src in _rows(W, H, lay, len(frames), base):
        buf[at:at + rw] = fr[k][src:src + rw]
    return buf


def sample_mask(W, H, lay, n, size, base=0):
    """True for the words of a `size`-byte buffer that hold samples."""
    m = np.zeros(size // 2, bool)
    for at, rw, _, _ in _rows(W, H, lay, n, base):
        m[at:at + rw] = True
    return m


def gather(W, H, buf, lay, n, base=0):
    out = [np.empty(W * H * 3 // 2, np.uint16) for _ in range(n)]
    for at, rw, k, dst in _rows(W, H, lay, n, base):
        out[k][dst:dst + rw] = buf[at:at + rw]
    return out
