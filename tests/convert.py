"""Test-side definitions for frames that go in as one format and come out as
another (include/mm.h "Different formats in and out"): NV12 / P010 codes in
with RGBA8 out, RGBA8 in with an NV12 code out.

A frame is what tests/ycbcr.py and tests/mmtest.py use: NV12 uint8
[H * 3 / 2][W], P010 uint16 words [H * 3 / 2][W], RGBA8 uint8 [H][W][4].
to_rgba() is a format's "in" rule (the RGBA frame a frame IS, unclamped),
store() a format's "out" rule, plain() the two in a row, float64 throughout:
what the first frame and apply_magnification = 0 give.  reference() is the
oracle (mmtest.oracle_run) on the in rule's float32 frames, stored by the out
rule; run() the same frames through Handle.process_convert /
process_stream_convert, tight or in a named Surface per side.
"""
import numpy as np

import mmtest as T
import ycbcr

RGBA8 = 0


def info(fmt):
    """-> (kind, matrix, full, depth): kind 'rgba8' or '420'."""
    if fmt == RGBA8:
        return "rgba8", None, None, None
    matrix = {0: 601, 32: 709, 64: 2020}[fmt & 96]
    base = fmt & ~96
    assert base in (16, 17, 18, 19), fmt
    return "420", matrix, bool(base & 1), 8 if base < 18 else 10


def to_rgba(frame, fmt, dtype=np.float32):
    """The "in" rule: the RGBA frame `frame` IS (alpha 1; a 4:2:0 frame unclamped)."""
    kind, matrix, full, depth = info(fmt)
    if kind == "rgba8":
        out = frame.astype(np.float64) / 255.0
        out[..., 3] = 1.0   # (the operator gives alpha weight 0; the out rules ignore it)
        return out.astype(dtype)
    return ycbcr.decode(frame, dtype, matrix=matrix, full=full, depth=depth)


def store(rgba, fmt):
    """The "out" rule on a float RGBA frame: saturate, then RGBA8
    floor(v * 255 + 0.5) with alpha 255, or the 4:2:0 code's encode."""
    kind, matrix, full, depth = info(fmt)
    f = np.clip(np.asarray(rgba)[..., :3].astype(np.float64), 0.0, 1.0)
    if kind == "rgba8":
        out = np.empty(f.shape[:2] + (4,), np.uint8)
        out[..., :3] = np.floor(f * 255.0 + 0.5).astype(np.uint8)
        out[..., 3] = 255
        return out
    return ycbcr.encode(f, matrix=matrix, full=full, depth=depth)


def plain(frame, in_fmt, out_fmt):
    """The plain conversion: the out rule applied to the in frame's RGBA frame."""
    return store(to_rgba(frame, in_fmt, np.float64), out_fmt)


def frames(W, H, n, fmt, stress=False, low_bits=False):
    """n synthetic frames of `fmt` (mmtest.synth's clip, encoded for a 4:2:0
    code).  stress: ycbcr.chroma_stress's gradient planes.  low_bits (P010):
    non-zero low 6 bits in every word (P016 content), a fixed pattern."""
    kind, matrix, full, depth = info(fmt)
    out = []
    for t, rgb in enumerate(T.synth(W, H, n, fmt="u8")):
        if kind == "rgba8":
            out.append(rgb)
            continue
        b = ycbcr.encode(rgb, matrix=matrix, full=full, depth=depth)
        if stress:
            b = ycbcr.chroma_stress(b, t, depth=depth)
        if low_bits:
            assert depth == 10
            yy, xx = np.mgrid[0:b.shape[0], 0:b.shape[1]]
            b = (b | ((yy * 7 + xx * 13 + t * 5) % 64).astype(np.uint16)).astype(np.uint16)
        out.append(b)
    return out


def reference(W, H, fr, in_fmt, out_fmt, L=5, S=25.0, edge=0, standard=None):
    """What the convert calls give: the plain conversion of the first frame,
    then the oracle's result on the in rule's float32 frames, stored by the out rule."""
    ref = T.oracle_run(W, H, [to_rgba(f, in_fmt, np.float32) for f in fr], L, S, edge, standard=standard)
    return [plain(fr[0], in_fmt, out_fmt)] + [store(r, out_fmt) for r in ref[1:]]


def out_frames(n, W, H, fmt):
    """A zeroed array for n tight output frames of `fmt`."""
    kind, _, _, depth = info(fmt)
    if kind == "rgba8":
        return np.zeros((n, H, W, 4), np.uint8)
    return np.zeros((n, H * 3 // 2, W), np.uint8 if depth == 8 else np.uint16)


def run(W, H, fr, in_fmt, out_fmt, L=5, S=25.0, edge=0, mode="frame", batch=8, apply=True, standard=None,
        extra=None, handle=None):
    """The frames through the convert entry points, tight on both sides.
    mode: 'frame' (single device calls), 'stream', 'host' (host-memory frames).
    handle: run on this Handle and leave it open (else a fresh one)."""
    import torch
    import mm355
    h = handle
    if h is None:
        extra = dict(extra or {})
        if standard is not None:
            extra.update(mode=mm355.MODE_STANDARD, **T._std_fields(standard))
        p = mm355.Params.make(levels=L, phase_scale=S, edge_mode=edge, apply_magnification=apply, **extra)
        h = mm355.Handle(W, H, p)
        h.set_batch(batch)
    li, lo = mm355.Surface.tight(W, H, in_fmt), mm355.Surface.tight(W, H, out_fmt)
    n = len(fr)
    if mode == "host":
        res = out_frames(n, W, H, out_fmt)
        for k in range(n):
            h.process_convert(np.ascontiguousarray(fr[k]), li, res[k], lo, on_device=False)
    else:
        # (moved as bytes: nothing depends on a 16-bit tensor type)
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
