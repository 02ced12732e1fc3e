"""mm_surface on the host: the layout helpers, mm_surface_bytes' validation and
the Python side's layout derivation.  None of it touches a GPU."""
import ctypes
import struct

import numpy as np
import pytest

import mm355
from mm355 import Surface

INVALID, UNSUPPORTED = -1, -2
RGBA = {mm355.RGBA8: 4, mm355.RGBA32F: 16, mm355.RGBA16F: 8, mm355.RGBA8_SRGB: 4}
YUV = {mm355.NV12: 1, mm355.NV12_FULL: 1, mm355.P010: 2, mm355.P010_FULL: 2}   # bytes per sample
FORMATS = list(RGBA) + list(YUV)
SIZES = [(2, 2), (98, 62), (1920, 1080), (8192, 8192)]


def _code(call):
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W,H", SIZES)
def test_tight_is_the_packed_layout(fmt, W, H):
    s = Surface.tight(W, H, fmt)
    rb = W * (RGBA.get(fmt) or YUV[fmt])
    assert s.format == fmt and s.pitch == rb
    if fmt in YUV:
        assert (s.chroma_offset, s.chroma_pitch) == (rb * H, rb)
    else:
        assert (s.chroma_offset, s.chroma_pitch) == (0, 0)
    assert s.frame_stride == mm355.frame_bytes(W, H, fmt)
    assert s.bytes(W, H) == mm355.frame_bytes(W, H, fmt)


def test_aligned_is_a_decoders_layout():
    s = Surface.aligned(1920, 1080, mm355.NV12, 256, 16)
    assert (s.pitch, s.chroma_offset, s.chroma_pitch, s.frame_stride) == (2048, 2048 * 1088, 2048, 2048 * 1632)
    assert s.bytes(1920, 1080) == 2048 * 1088 + 539 * 2048 + 1920
    # P010: rows of 3840 bytes are a multiple of 256 already; 1088 + 544 padded rows
    s = Surface.aligned(1920, 1080, mm355.P010, 256, 16)
    assert (s.pitch, s.chroma_offset, s.chroma_pitch, s.frame_stride) == (3840, 3840 * 1088, 3840, 3840 * 1632)
    # RGBA8: 7680 = 30 x 256; one plane of 1088 padded rows
    s = Surface.aligned(1920, 1080, mm355.RGBA8, 256, 16)
    assert (s.pitch, s.chroma_offset, s.chroma_pitch, s.frame_stride) == (7680, 0, 0, 7680 * 1088)
    assert s.bytes(1920, 1080) == 7680 * 1079 + 7680
    # a width that the alignment does round: 200 x 120 RGBA8, 800 -> 1024, 120 -> 128 rows
    s = Surface.aligned(200, 120, mm355.RGBA8, 256, 16)
    assert (s.pitch, s.frame_stride, s.bytes(200, 120)) == (1024, 1024 * 128, 1024 * 119 + 800)
    # 4:2:0 needs an even row alignment; the pitch alignment is a multiple of the unit
    assert _code(lambda: Surface.aligned(64, 48, mm355.NV12, 256, 3)) == INVALID
    assert _code(lambda: Surface.aligned(64, 48, mm355.P010, 6, 2)) == INVALID
    assert Surface.aligned(64, 48, mm355.RGBA8, 256, 3).frame_stride == 256 * 48


def _nv12(W, H, **kw):
    s = Surface.tight(W, H, mm355.NV12)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_validation_rules():
    W, H = 64, 48
    ok = Surface(format=mm355.RGBA8, pitch=W * 4 + 4)
    assert ok.bytes(W, H) == (W * 4 + 4) * (H - 1) + W * 4      # not pitch * H
    # format
    assert _code(lambda: Surface(format=7, pitch=W * 4).bytes(W, H)) == INVALID
    assert _code(lambda: Surface.tight(W, H, 7)) == INVALID
    # odd 4:2:0 size, as mm_frame_bytes
    assert _code(lambda: _nv12(W, H).bytes(W - 1, H)) == UNSUPPORTED
    assert _code(lambda: Surface.tight(W, H - 1, mm355.P010)) == UNSUPPORTED
    assert _code(lambda: mm355.frame_bytes(W - 1, H, mm355.NV12)) == UNSUPPORTED
    # pitch below the row bytes; not a multiple of the unit (every unit)
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=W * 4 - 4).bytes(W, H)) == INVALID
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=W * 4 + 2).bytes(W, H)) == INVALID
    assert _code(lambda: Surface(format=mm355.RGBA32F, pitch=W * 16 + 8).bytes(W, H)) == INVALID
    assert _code(lambda: Surface(format=mm355.RGBA16F, pitch=W * 8 + 4).bytes(W, H)) == INVALID
    assert _code(lambda: _nv12(W, H, pitch=W + 1, chroma_offset=(W + 1) * H + 1).bytes(W, H)) == INVALID
    assert _code(lambda: Surface(format=mm355.P010, pitch=2 * W + 2, chroma_offset=(2 * W + 2) * H,
                                 chroma_pitch=2 * W).bytes(W, H)) == INVALID
    # the same for the chroma pitch and the chroma offset
    assert _code(lambda: _nv12(W, H, chroma_pitch=W - 2).bytes(W, H)) == INVALID
    assert _code(lambda: _nv12(W, H, chroma_pitch=W + 1).bytes(W, H)) == INVALID
    assert _code(lambda: _nv12(W, H, chroma_offset=W * H + 1).bytes(W, H)) == INVALID
    # chroma plane overlapping the last luma row's samples; right behind them is fine
    assert _code(lambda: _nv12(W, H, chroma_offset=W * H - 2).bytes(W, H)) == INVALID
    assert _nv12(W, H, pitch=W + 6, chroma_offset=(W + 6) * (H - 1) + W).bytes(W, H) == \
        (W + 6) * (H - 1) + W + W * (H // 2)
    # chroma fields on an RGBA format
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=W * 4, chroma_offset=W * 4 * H).bytes(W, H)) == INVALID
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=W * 4, chroma_pitch=W * 4).bytes(W, H)) == INVALID
    # every tight layout the project takes today passes
    assert Surface.tight(98, 62, mm355.NV12).bytes(98, 62) == 98 * 62 * 3 // 2


def test_extent_bound_and_overflow():
    # the kernels' 32-bit byte offsets reach extent <= 2^32: both sides of the bound
    assert Surface(format=mm355.RGBA8, pitch=2 ** 32 - 8).bytes(2, 2) == 2 ** 32
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=2 ** 32 - 4).bytes(2, 2)) == UNSUPPORTED
    s = _nv12(64, 48, chroma_offset=2 ** 32 - 64 * 24)
    assert s.bytes(64, 48) == 2 ** 32
    s.chroma_offset += 2
    assert _code(lambda: s.bytes(64, 48)) == UNSUPPORTED
    # arithmetic overflow of size_t
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=2 ** 63).bytes(2, 4)) == INVALID
    assert _code(lambda: Surface(format=mm355.RGBA8, pitch=2 ** 64 - 4).bytes(2, 2)) == INVALID
    assert _code(lambda: _nv12(64, 48, chroma_offset=2 ** 64 - 64).bytes(64, 48)) == INVALID
    assert _code(lambda: _nv12(64, 48, chroma_pitch=2 ** 62).bytes(64, 48)) == INVALID
    assert _code(lambda: Surface.aligned(64, 48, mm355.RGBA8, 2 ** 63, 16)) == INVALID


def test_struct_layout_matches_the_library():
    """The ctypes mirror against what the library writes and reads through a
    raw buffer: mm_surface's size and field offsets."""
    lib = mm355.lib()
    size = ctypes.sizeof(Surface)
    offs = [getattr(Surface, f).offset for f, _ in Surface._fields_]
    assert (size, offs) == (40, [0, 8, 16, 24, 32])
    # written by the library: distinct values in every field, nothing past the struct
    raw = (ctypes.c_ubyte * 64)(*([0xEE] * 64))
    fill = lib.mm_surface_aligned
    assert fill(200, 120, mm355.P010, 256, 16, ctypes.cast(raw, ctypes.POINTER(Surface))) == 0
    b = bytes(raw)
    assert struct.unpack_from("<i", b, 0)[0] == mm355.P010
    assert struct.unpack_from("<QQQQ", b, 8) == (512, 512 * 128, 512, 512 * 192)
    assert b[size:] == b"\xEE" * (64 - size)
    # read by the library: a layout whose four size_t fields all differ
    W, H = 64, 48
    raw = struct.pack("<i4xQQQQ", mm355.NV12, W + 2, (W + 2) * H + 6, W + 10, 1 << 20)
    n = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(raw)
    assert lib.mm_surface_bytes(W, H, ctypes.cast(buf, ctypes.POINTER(Surface)), ctypes.byref(n)) == 0
    assert n.value == (W + 2) * H + 6 + (W + 10) * (H // 2 - 1) + W
    assert mm355.lib().mm_abi_version() == 10 and mm355.has_surfaces()
    assert {"mm_surface_tight", "mm_surface_aligned", "mm_surface_bytes", "mm_process_surface",
            "mm_process_stream_surfaces", "mm_compute_state_surface"} <= set(mm355.abi_symbols())


class _Recorder:
    """Stands in for the handle: records what OnRenderImage would call."""

    def __init__(self):
        self.calls = []

    def process(self, *a, **kw):
        self.calls.append(("process", a, kw))

    def process_surface(self, *a, **kw):
        self.calls.append(("process_surface", a, kw))


def test_processor_derives_the_layout_from_numpy_strides():
    W, H = 64, 48
    parent = np.zeros((100, 90, 4), np.uint8)
    out = np.zeros((H, W, 4), np.uint8)
    roi = parent[7:7 + H, 5:5 + W]
    lay = mm355.frame_layout(roi, W, H, mm355.RGBA8)
    assert (lay.format, lay.pitch, lay.chroma_offset, lay.chroma_pitch) == (mm355.RGBA8, 90 * 4, 0, 0)
    assert mm355.frame_layout(out, W, H, mm355.RGBA8) is None              # contiguous: the tight call
    pf = np.zeros((60, 70, 4), np.float32)
    assert mm355.frame_layout(pf[3:3 + H, 1:1 + W], W, H, mm355.RGBA32F).pitch == 70 * 16
    proc = mm355.MotionMagnificationProcessor(W, H)
    proc._handle = rec = _Recorder()
    proc.OnRenderImage(roi, out)
    name, a, kw = rec.calls[-1]
    assert name == "process_surface" and a[0] is roi and a[2] is out and kw["on_device"] is False
    assert a[1].pitch == 360 and a[3].pitch == W * 4                       # each side its own layout
    proc.OnRenderImage(out.copy(), out)
    assert rec.calls[-1][0] == "process"
    # anything else still raises: column-strided, channel-strided, reversed rows, wrong shape
    wide = np.zeros((H, 2 * W, 4), np.uint8)
    deep = np.zeros((H, W, 8), np.uint8)
    for bad in (wide[:, ::2], deep[:, :, ::2], out[::-1], parent[:H, :W + 1]):
        with pytest.raises(mm355.MMError) as ei:
            proc.OnRenderImage(bad, out)
        assert ei.value.code == INVALID
        with pytest.raises(mm355.MMError):
            proc.OnRenderImage(out, bad)
    assert len(rec.calls) == 2
    proc._handle = None
