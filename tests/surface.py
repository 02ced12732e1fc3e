"""Helpers for the pitched-surface tests (mm_surface, include/mm.h).

A frame is handled as its tight bytes (a flat uint8 array of mm_frame_bytes),
whatever the format; scatter() places the W x H samples of such frames into a
pitched buffer, gather() reads them back, and sample_mask() marks which bytes
of the buffer are samples, so that a test can hold every other byte (row tails,
the gap between the planes and between frames, whatever surrounds a region of
interest) to the value it had before the call.
"""
import functools
import os

import numpy as np

import mmtest as T
import nv12
import p010

L, S = 5, 25.0
POISON = 0xFF      # input padding: NaN for the float formats, out-of-range video codes
TAIL = 64          # bytes kept after the last frame's extent (padding like any other)


class env:
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


def fmt_code(name):
    import mm355
    return {"rgba8": mm355.RGBA8, "rgba32f": mm355.RGBA32F, "rgba16f": mm355.RGBA16F,
            "srgb8": mm355.RGBA8_SRGB, "nv12": mm355.NV12, "nv12_full": mm355.NV12_FULL,
            "p010": mm355.P010, "p010_full": mm355.P010_FULL}[name]


def is420(name):
    return name.startswith(("nv12", "p010"))


def sample_bytes(name):
    """Bytes of one row element: an RGBA pixel, or one 4:2:0 sample."""
    return {"rgba8": 4, "srgb8": 4, "rgba16f": 8, "rgba32f": 16}.get(name, 2 if name.startswith("p010") else 1)


def unit(name):
    """What pitches, offsets, strides and frame pointers are multiples of."""
    return {"nv12": 2, "nv12_full": 2, "p010": 4, "p010_full": 4}.get(name, sample_bytes(name))


def row_bytes(name, W):
    return W * sample_bytes(name)


def planes(name, W, H, lay):
    """[(offset in the frame, pitch, rows, row bytes, offset in the tight frame)]."""
    rb = row_bytes(name, W)
    out = [(0, lay.pitch, H, rb, 0)]
    if is420(name):
        out.append((lay.chroma_offset, lay.chroma_pitch, H // 2, rb, rb * H))
    return out


@functools.lru_cache(maxsize=None)
def tight_frames(name, W, H, n, gray=False):
    """n synthetic frames of the format, each as its tight bytes (read-only)."""
    out = []
    for rgb in T.synth(W, H, n, fmt="u8", gray=gray):
        if name in ("rgba8", "srgb8"):
            a = rgb
        elif name == "rgba32f":
            a = rgb.astype(np.float32) / np.float32(255)
        elif name == "rgba16f":
            a = (rgb.astype(np.float32) / np.float32(255)).astype(np.float16)
        elif name.startswith("nv12"):
            a = nv12.encode(rgb, full=name.endswith("full"))
        else:
            a = p010.encode(rgb, full=name.endswith("full"))
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def typed(name, W, H, flat):
    """A tight frame's bytes in the array form the other tests' helpers take."""
    if name in ("rgba8", "srgb8"):
        return flat.reshape(H, W, 4)
    if name == "rgba32f":
        return flat.view(np.float32).reshape(H, W, 4)
    if name == "rgba16f":
        return flat.view(np.float16).reshape(H, W, 4)
    if name.startswith("nv12"):
        return flat.reshape(H * 3 // 2, W)
    return flat.view(np.uint16).reshape(H * 3 // 2, W)


# ---- layouts -----------------------------------------------------------------
def lay_tight(name, W, H):
    import mm355
    return mm355.Surface.tight(W, H, fmt_code(name))


def lay_plus_unit(name, W, H):
    """(a) pitch = row bytes + one unit: breaks every wider alignment."""
    import mm355
    rb, u = row_bytes(name, W), unit(name)
    s = mm355.Surface(format=fmt_code(name), pitch=rb + u)
    if is420(name):
        s.chroma_offset, s.chroma_pitch = (rb + u) * H, rb + u
    s.frame_stride = s.bytes(W, H) + u
    return s


def lay_aligned(name, W, H):
    """(b) a decoder's layout."""
    import mm355
    return mm355.Surface.aligned(W, H, fmt_code(name), 256, 16)


def lay_split_chroma(name, W, H):
    """(c) 4:2:0 with chroma_pitch != pitch and the chroma plane at 2 mod 4
    (NV12) / 4 mod 8 (P010) from the base."""
    import mm355
    rb, u = row_bytes(name, W), unit(name)
    s = mm355.Surface(format=fmt_code(name), pitch=rb + 2 * u, chroma_pitch=rb + 6 * u)
    off = (rb + 2 * u) * H + 4 * u
    while off % (2 * u) != u:
        off += u
    s.chroma_offset = off
    s.frame_stride = (s.bytes(W, H) + 7) // 8 * 8
    return s


def lay_stride_plus_unit(name, W, H):
    """(d) tight frames one alignment unit apart more than their extent:
    consecutive frames of a stream alternate alignment."""
    s = lay_tight(name, W, H)
    s.frame_stride = s.bytes(W, H) + unit(name)
    return s


def lay_roi(name, W, H, PW, PH, x, y):
    """(e) the W x H region at (x, y) of a tight PW x PH parent: (layout, byte
    offset of the region's first sample in the parent, the parent's bytes)."""
    import mm355
    sb = sample_bytes(name)
    pp = PW * sb
    s = mm355.Surface(format=fmt_code(name), pitch=pp)
    base = y * pp + x * sb
    size = pp * PH
    if is420(name):
        assert x % 2 == 0 and y % 2 == 0
        s.chroma_pitch = pp
        s.chroma_offset = pp * PH + (y // 2) * pp + x * sb - base
        size += pp * PH // 2
    s.frame_stride = size
    return s, base, size


# ---- buffers -------------------------------------------------------------------
def buffer_bytes(name, W, H, lay, n, base=0):
    return base + (n - 1) * lay.frame_stride + lay.bytes(W, H) + TAIL


def scatter(name, W, H, frames, lay, base=0, fill=POISON, size=None):
    """Tight frames -> one pitched buffer (uint8), every other byte `fill`."""
    buf = np.full(size or buffer_bytes(name, W, H, lay, len(frames), base), fill, np.uint8)
    for k, f in enumerate(frames):
        at = base + k * lay.frame_stride
        for off, pitch, rows, rb, src in planes(name, W, H, lay):
            for r in range(rows):
                buf[at + off + r * pitch: at + off + r * pitch + rb] = f[src + r * rb: src + (r + 1) * rb]
    return buf


def sample_mask(name, W, H, lay, n, size, base=0):
    m = np.zeros(size, bool)
    for k in range(n):
        at = base + k * lay.frame_stride
        for off, pitch, rows, rb, _ in planes(name, W, H, lay):
            for r in range(rows):
                m[at + off + r * pitch: at + off + r * pitch + rb] = True
    return m


def gather(name, W, H, buf, lay, n, base=0):
    out = []
    for k in range(n):
        at = base + k * lay.frame_stride
        f = np.empty(sum(rows * rb for _, _, rows, rb, _ in planes(name, W, H, lay)), np.uint8)
        for off, pitch, rows, rb, dst in planes(name, W, H, lay):
            for r in range(rows):
                f[dst + r * rb: dst + (r + 1) * rb] = buf[at + off + r * pitch: at + off + r * pitch + rb]
        out.append(f)
    return out


def sentinel(size):
    """The output buffers' fill: a byte pattern no kernel output reproduces by chance."""
    return ((np.arange(size, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)


def make_params(edge=0, apply=True, standard=None, debug=None, extra=None):
    import mm355
    extra = dict(extra or {})
    if standard is not None:
        extra.update(mode=mm355.MODE_STANDARD, **T._std_fields(standard))
    if debug is not None:
        extra.update(show_magnitude=debug[0], show_phase=debug[1])
    return mm355.Params.make(levels=L, phase_scale=S, edge_mode=edge, apply_magnification=apply, **extra)


def run_pitched(name, W, H, frames, lin, lout, mode="frame", batch=8, in_base=0, out_base=0,
                in_size=None, out_size=None, params=None, profile=False):
    """The frames through the pitched entry points: the input scattered into a
    poisoned buffer in layout `lin`, the output buffer pre-filled with the
    sentinel.  mode: "frame" (mm_process_surface per frame, device), "stream"
    (mm_process_stream_surfaces) or "host" (mm_process_surface on numpy
    memory).  Returns the gathered tight output frames, after asserting that
    every byte of the output buffer that is no sample still holds the sentinel
    (and the launch counts when profile is set)."""
    import torch
    import mm355
    n = len(frames)
    src = scatter(name, W, H, frames, lin, in_base, size=in_size)
    out_size = out_size or buffer_bytes(name, W, H, lout, n, out_base)
    sent = sentinel(out_size)
    h = mm355.Handle(W, H, params or make_params())
    h.set_batch(batch)
    prof = None
    if mode == "host":
        res = sent.copy()
        for k in range(n):
            h.process_surface(src[in_base + k * lin.frame_stride:], lin,
                              res[out_base + k * lout.frame_stride:], lout, on_device=False)
    else:
        a = torch.from_numpy(src).cuda()
        b = torch.from_numpy(sent).cuda()
        assert a.data_ptr() % 256 == 0 and b.data_ptr() % 256 == 0
        if profile:
            h.profile_begin()
        if mode == "stream":
            h.process_stream_surfaces(a[in_base:], lin, b[out_base:], lout, n)
        else:
            for k in range(n):
                h.process_surface(a[in_base + k * lin.frame_stride:], lin,
                                  b[out_base + k * lout.frame_stride:], lout)
        if profile:
            prof = h.profile_end()
        torch.cuda.synchronize()
        res = b.cpu().numpy()
    h.close()
    keep = ~sample_mask(name, W, H, lout, n, out_size, out_base)
    bad = np.flatnonzero(keep & (res != sent))
    assert bad.size == 0, f"{bad.size} padding bytes written, first at {bad[:8]}"
    got = gather(name, W, H, res, lout, n, out_base)
    return (got, prof) if profile else got


def run_tight(name, W, H, frames, mode="frame", batch=8, **kw):
    """The same frames through the tight entry points (mmtest.gpu_run), as bytes."""
    arr = [typed(name, W, H, f) for f in frames]
    if name.startswith("p010"):
        arr = [a.view(np.uint8) for a in arr]
    got = T.gpu_run(W, H, arr, L, S, mode=mode, batch=batch, fmt=fmt_code(name), **kw)
    return [np.ascontiguousarray(g).view(np.uint8).reshape(-1) for g in got]


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, k, int((g != w).sum()))
