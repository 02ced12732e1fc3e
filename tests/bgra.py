"""Test-side helpers of the B G R A formats (MM_BGRA8 / MM_BGRA8_SRGB, include/mm.h):
swap(), the synthetic clips with a non-trivial alpha plane, the runners on the
BGRA path and on its RGBA8 twin, and the pitched-buffer helpers their tests share.

A frame is one array [H][W][4] of uint8.  A BGRA frame IS the MM_RGBA8 (or
MM_RGBA8_SRGB) frame with bytes 0 and 2 of every pixel exchanged: swap() makes
the one from the other, and every check is bitwise against the RGBA8 path on the
same GPU, which the existing suites hold to the oracle.
"""
import functools
import os

import numpy as np

import mmtest as T

L, S = 5, 25.0
POISON = 0xFF


def twin_fmt(fmt):
    """The RGBA code a BGRA code is the byte exchange of."""
    import mm355
    return {mm355.BGRA8: mm355.RGBA8, mm355.BGRA8_SRGB: mm355.RGBA8_SRGB}[fmt]


def swap(f):
    """Bytes 0 and 2 of every pixel exchanged (R G B A <-> B G R A), a contiguous copy."""
    return np.ascontiguousarray(np.asarray(f)[..., [2, 1, 0, 3]])


@functools.lru_cache(maxsize=None)
def frames(W, H, n):
    """n R G B A frames of the project's synthetic stream (mmtest.synth's u8
    frames) with a non-trivial alpha plane in place of its 255, read-only: a
    passthrough has to carry it, the operator has to ignore it."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for t, f in enumerate(T.synth(W, H, n, fmt="u8")):
        f = np.array(f, dtype=np.uint8, order="C")
        f[..., 3] = ((yy * 5 + xx * 3 + t * 11) % 256).astype(np.uint8)
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


class env:
    """Environment switches of the library (MM_K34_ROWS ...), read at mm_create."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(W, H, fr, fmt, *a, **kw):
    """T.gpu_run on R G B A frames sent as B G R A frames of `fmt`; the result as it
    comes back (B G R A)."""
    return T.gpu_run(W, H, [swap(f) for f in fr], *a, fmt=fmt, **kw)


def run_twin(W, H, fr, fmt, *a, **kw):
    """swap() of the RGBA path's result on the same R G B A frames: what identity 1
    says run() returns."""
    return [swap(g) for g in T.gpu_run(W, H, list(fr), *a, fmt=twin_fmt(fmt), **kw)]


def same(a, b, what):
    assert len(a) == len(b), what
    for k in range(len(a)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))


def ran(got, sent, what=""):
    """The operator ran on the frames after the first: more than half of the
    colour bytes differ from the input."""
    for k in range(1, len(got)):
        assert (np.asarray(got[k])[..., :3] != np.asarray(sent[k])[..., :3]).mean() > 0.5, (what, k)


# ---- convert pairs -------------------------------------------------------------
def out_frames(n, W, H, fmt):
    import mm355
    if fmt in (mm355.RGBA8, mm355.BGRA8):
        return np.zeros((n, H, W, 4), np.uint8)
    return np.zeros((n, H * 3 // 2, W), np.uint16 if (fmt & ~96) in (18, 19) else np.uint8)


def convert(W, H, fr, in_fmt, out_fmt, mode="frame", batch=8, apply=True, handle=None):
    """The frames through the convert entry points, tight on both sides (tests/
    convert.py's run for pairs with a BGRA side).  mode: 'frame' or 'stream'."""
    import torch
    import mm355
    h = handle
    if h is None:
        h = mm355.Handle(W, H, mm355.Params.make(levels=L, phase_scale=S, apply_magnification=apply))
        h.set_batch(batch)
    li, lo = mm355.Surface.tight(W, H, in_fmt), mm355.Surface.tight(W, H, out_fmt)
    n = len(fr)
    src = torch.from_numpy(np.ascontiguousarray(np.stack(fr)).view(np.uint8)).cuda()
    dst = torch.from_numpy(out_frames(n, W, H, out_fmt)).cuda()
    if mode == "frame":
        for k in range(n):
            h.process_convert(src[k], li, dst[k], lo)
    else:
        h.process_stream_convert(src, li, dst, lo, n)
    torch.cuda.synchronize()
    res = dst.cpu().numpy()
    if handle is None:
        h.close()
    return list(res)


# ---- pitched buffers -----------------------------------------------------------
def scatter(fr, pitch, stride, size, base=0):
    """Tight frames [H][W][4] -> one pitched uint8 buffer (frame k at base +
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
            m[at:at + 4 * W] = True
    return m


def gather(buf, W, H, n, pitch, stride, base=0):
    out = []
    for k in range(n):
        rows = [buf[base + k * stride + r * pitch: base + k * stride + r * pitch + 4 * W] for r in range(H)]
        out.append(np.stack(rows).reshape(H, W, 4))
    return out


def sentinel(size):
    return ((np.arange(size, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
