"""Test-side codec for the v210 format of include/mm.h (MM_V210, its _FULL code
and the matrix bits), in numpy.  A V210 frame IS the MM_Y210 frame whose words
are code << 6, so everything about codes, ranges and matrices is tests/y210.py's;
this module only moves the codes between the two layouts.

A frame is uint32 [H][pitch / 4] with pitch = 128 ceil(W / 48): each dword holds
three 10-bit codes in bits 0-9, 10-19, 20-29, a row is the sample sequence
Cb Y0 Cr Y1 Cb Y2 Cr Y3 ... (2 W samples) three to a dword, D(W) = 4 (W / 6) +
{0, 2, 3}[(W % 6) / 2] dwords; the dwords past D(W) are padding.

Pinned to the vector of include/mm.h (samples 1 .. 12 give 0x00300801,
0x00601404, 0x00902007, 0x00C02C0A), to host/v210.c (tests/test_v210_host.py
holds the two against each other) and to tests/y210.py's frame shape.

The surface helpers at the end handle the one-plane layout with unit 16, on
frames as their used bytes (flat uint8 arrays of 4 D(W) H bytes).
"""
import numpy as np

import ycbcr

UNIT = 16     # one group: what pitches, strides and frame pointers are multiples of
TAIL = 64     # bytes kept after the last frame's extent
PACK = 4096   # MM_PACK_V210


def fmt_code(matrix=601, full=False):
    """The format code of include/mm.h."""
    return (22 | PACK) + (1 if full else 0) + ycbcr.matrix_bit(matrix)


def dwords(W):
    """D(W): the used dwords of a row."""
    return 4 * (W // 6) + (0, 2, 3)[(W % 6) // 2]


def row_bytes(W):
    return 4 * dwords(W)


def pitch(W):
    return 128 * ((W + 47) // 48)


def frame_bytes(W, H):
    return pitch(W) * H


def _sequence(y210_frame):
    """Y210 frame [H][2 W] (words Y0 Cb Y1 Cr) -> the samples in v210's order Cb Y0 Cr Y1."""
    H, n = y210_frame.shape
    return y210_frame.reshape(H, n // 4, 4)[:, :, [1, 0, 3, 2]].reshape(H, n)


def pack(y210_frame, pad=0, stray=None):
    """Y210 frame uint16 [H][2 W] -> v210 frame uint32 [H][pitch / 4], codes =
    word >> 6, unused fields zero, every padding dword `pad`.  stray: a
    generator whose random bits go into bits 30-31 of every used dword and into
    the unused fields of a partial last group's dwords."""
    assert y210_frame.dtype == np.uint16 and y210_frame.ndim == 2 and y210_frame.shape[1] % 4 == 0
    H, W = y210_frame.shape[0], y210_frame.shape[1] // 2
    D = dwords(W)
    s = np.zeros((H, 3 * D), np.uint32)
    used = np.zeros(3 * D, bool)
    used[:2 * W] = True
    s[:, :2 * W] = _sequence(y210_frame) >> 6
    if stray is not None:
        s[:, ~used] = stray.integers(0, 1024, (H, int((~used).sum())), dtype=np.uint32)
    s = s.reshape(H, D, 3)
    d = s[..., 0] | s[..., 1] << 10 | s[..., 2] << 20
    if stray is not None:
        d |= stray.integers(0, 4, (H, D), dtype=np.uint32) << 30
    out = np.full((H, pitch(W) // 4), pad, np.uint32)
    out[:, :D] = d
    return out


def unpack(v210_frame, W):
    """v210 frame uint32 [H][>= D(W)] -> Y210 frame uint16 [H][2 W], words code << 6."""
    assert v210_frame.dtype == np.uint32 and v210_frame.ndim == 2
    H, D = v210_frame.shape[0], dwords(W)
    d = v210_frame[:, :D]
    s = np.stack([d & 1023, (d >> 10) & 1023, (d >> 20) & 1023], axis=2).reshape(H, 3 * D)[:, :2 * W]
    out = np.empty((H, 2 * W), np.uint16)
    out.reshape(H, W // 2, 4)[:, :, [1, 0, 3, 2]] = (s << 6).astype(np.uint16).reshape(H, W // 2, 4)
    return out


def used(v210_frame, W):
    """The used dwords [H][D(W)] of a frame."""
    return v210_frame[:, :dwords(W)]


def clean(v210_frame, W):
    """The frame's used dwords as the library writes them: bits 30-31 and the
    unused fields of a partial last group zero."""
    return used(pack(unpack(v210_frame, W)), W)


# ---- surfaces: one plane, unit 16 --------------------------------------------------
def flat(v210_frame, W):
    """The used bytes of a frame, rows back to back: uint8 [4 D(W) H]."""
    return np.ascontiguousarray(used(v210_frame, W)).view(np.uint8).reshape(-1)


def unflat(buf, W, H):
    """flat()'s inverse: uint32 [H][D(W)]."""
    return np.ascontiguousarray(buf).view(np.uint32).reshape(H, dwords(W))


def buffer_bytes(W, H, lay, n, base=0):
    return base + (n - 1) * lay.frame_stride + lay.bytes(W, H) + TAIL


def scatter(W, H, frames, lay, base=0, fill=0xFF, size=None):
    """Frames as their used bytes (flat()) -> one pitched buffer, every other byte `fill`."""
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
