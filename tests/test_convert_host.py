"""Different formats in and out, on the host: mm_convert_supported's table, the
layout rules each side of a pair goes by, OnRenderImage(dst_fmt=)'s refusals and
the numpy definitions of the plain conversion (tests/convert.py) on hand-computed
pixels.  None of it touches a GPU, and so none of it holds a handle: a convert
call's validation of each layout, and mm_process_surface's MM_ERR_INVALID for
differing formats past the NULL-handle check, are in test_convert.py.  The layout
rules and the numpy definitions are not new and pass without the feature."""
import ctypes

import numpy as np
import pytest

import convert as C
import mm355
from mm355 import Surface

OK, INVALID, UNSUPPORTED = 0, -1, -2
NV12_CODES = (16, 17, 48, 49, 80, 81)
P010_CODES = (18, 19, 50, 51, 82, 83)
VALID = (0, 1, 2, 3, 8, 9, 10, 11, 13, 141, 22, 23, 24, 25, 26, 27, 54, 56, 58) + NV12_CODES + P010_CODES


def _code(call):
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def test_symbols_are_declared_and_built():
    assert {"mm_convert_supported", "mm_process_convert", "mm_process_stream_convert"} <= set(mm355.abi_symbols())
    assert mm355.has_convert() and mm355.lib().mm_abi_version() == 10
    for name in mm355.binding.CONVERT_SYMBOLS:
        assert hasattr(mm355.lib(), name), name


def test_supported_table():
    for c in NV12_CODES + P010_CODES:
        assert mm355.convert_supported(c, mm355.RGBA8) == OK, c          # decode
    for c in NV12_CODES:
        assert mm355.convert_supported(mm355.RGBA8, c) == OK, c          # encode
    for c in VALID:
        assert mm355.convert_supported(c, c) == OK, c                    # the existing calls
    for a, b in ((mm355.RGBA8, mm355.P010), (mm355.NV12, mm355.RGBA32F), (mm355.YUY2, mm355.RGBA8),
                 (mm355.RGB24, mm355.BGR24), (mm355.NV12, mm355.P010), (mm355.NV12, mm355.NV12 | 32),
                 (mm355.NV12, mm355.NV12_FULL), (mm355.RGBA8_SRGB, mm355.NV12), (mm355.NV12, mm355.RGBA8_SRGB),
                 (mm355.Y8, mm355.RGBA8), (mm355.RGBA8, mm355.Y8), (mm355.Y210, mm355.RGBA8),
                 (mm355.P010, mm355.RGBA16F), (mm355.RGBA8, mm355.RGB24), (mm355.BGR24, mm355.RGBA8)):
        assert mm355.convert_supported(a, b) == UNSUPPORTED, (a, b)
    # every other pair of two valid codes, exhaustively
    for a in VALID:
        for b in VALID:
            want = OK if a == b or (a in NV12_CODES + P010_CODES and b == 0) or (a == 0 and b in NV12_CODES) \
                else UNSUPPORTED
            assert mm355.convert_supported(a, b) == want, (a, b)
    for bad in (14, 20, mm355.RGBA8 | 128, mm355.RGBA8 | mm355.MATRIX_BT709, -1, 16 | 96, 256, 13 | 32):
        assert mm355.convert_supported(bad, mm355.RGBA8) == INVALID, bad
        assert mm355.convert_supported(mm355.NV12, bad) == INVALID, bad
        assert mm355.convert_supported(bad, bad) == INVALID, bad


def test_null_arguments_and_the_old_entry_points():
    lib = mm355.lib()
    li, lo = Surface.tight(64, 48, mm355.NV12), Surface.tight(64, 48, mm355.RGBA8)
    buf = ctypes.create_string_buffer(64 * 48 * 4)
    for fn in (lib.mm_process_convert, lib.mm_process_stream_convert, lib.mm_process_surface,
               lib.mm_process_stream_surfaces):
        assert fn(None, buf, ctypes.byref(li), buf, ctypes.byref(lo), 1, None) == INVALID


def test_surface_rules_the_two_sides_differ_by():
    """The existing layout rules (mm_surface_bytes / mm_frame_bytes) a convert
    call applies to each side; it passes without the feature.  The call's own
    validation needs a handle, so a GPU: test_convert.py::test_refusals_leave_the_next_output_unchanged."""
    W, H = 64, 48
    # NV12's unit is 2, RGBA8's 4: a pitch of W + 2 is a layout of the one and not of the other
    s = Surface.tight(W, H, mm355.NV12)
    s.pitch, s.chroma_offset = W + 2, (W + 2) * H
    assert s.bytes(W, H) == (W + 2) * H + W * (H // 2 - 1) + W
    s.pitch = W + 1
    assert _code(lambda: s.bytes(W, H)) == INVALID
    r = Surface.tight(W, H, mm355.RGBA8)
    r.pitch = 4 * W + 2
    assert _code(lambda: r.bytes(W, H)) == INVALID
    r.pitch, r.chroma_offset = 4 * W, 8           # an RGBA8 side has no chroma plane
    assert _code(lambda: r.bytes(W, H)) == INVALID
    # the union of the restrictions: 4:2:0 sides are even-sized
    assert _code(lambda: Surface.tight(97, 63, mm355.NV12)) == UNSUPPORTED
    assert Surface.tight(97, 63, mm355.RGBA8).pitch == 4 * 97
    # each side's own frame size
    assert mm355.frame_bytes(W, H, mm355.NV12) == W * H * 3 // 2 and mm355.frame_bytes(W, H, mm355.P010) == W * H * 3
    assert mm355.frame_bytes(W, H, mm355.RGBA8) == W * H * 4


class _Recorder:
    """Stands in for the handle: records what OnRenderImage would call."""

    def __init__(self):
        self.calls = []

    def process(self, *a, **kw):
        self.calls.append(("process", a, kw))

    def process_surface(self, *a, **kw):
        self.calls.append(("process_surface", a, kw))

    def process_convert(self, *a, **kw):
        self.calls.append(("process_convert", a, kw))


def test_on_render_image_checks_each_side_by_its_format():
    W, H = 64, 48
    proc = mm355.MotionMagnificationProcessor(W, H)
    proc._handle = rec = _Recorder()
    nv = np.zeros((H * 3 // 2, W), np.uint8)
    pw = np.zeros((H * 3 // 2, W), np.uint16)
    rgba = np.zeros((H, W, 4), np.uint8)
    try:
        # decode: the source by the 4:2:0 code, the destination by RGBA8
        proc.OnRenderImage(nv, rgba, fmt=mm355.NV12 | mm355.MATRIX_BT709, dst_fmt=mm355.RGBA8)
        name, a, kw = rec.calls[-1]
        assert name == "process_convert" and a[0] is nv and a[2] is rgba and kw["on_device"] is False
        assert (a[1].format, a[1].pitch, a[1].chroma_offset) == (48, W, W * H)
        assert (a[3].format, a[3].pitch, a[3].chroma_offset) == (0, 4 * W, 0)
        proc.OnRenderImage(pw, rgba, fmt=mm355.P010, dst_fmt=mm355.RGBA8)
        assert rec.calls[-1][1][1].pitch == 2 * W
        # encode: fmt from the dtype, a row-strided RGBA8 source keeps its own layout
        parent = np.zeros((100, 90, 4), np.uint8)
        proc.OnRenderImage(parent[7:7 + H, 5:5 + W], nv, dst_fmt=mm355.NV12_FULL)
        name, a, kw = rec.calls[-1]
        assert name == "process_convert" and (a[1].format, a[1].pitch) == (0, 360) and a[3].format == 17
        # dst_fmt None or equal to the source's format: today's calls
        proc.OnRenderImage(rgba, rgba.copy())
        assert rec.calls[-1][0] == "process"
        proc.OnRenderImage(rgba, rgba.copy(), dst_fmt=mm355.RGBA8)
        assert rec.calls[-1][0] == "process"
        n = len(rec.calls)
        bad = [
            (nv, np.zeros((H, W, 3), np.uint8), mm355.NV12, mm355.RGBA8),           # destination shape
            (nv, np.zeros((H, W, 4), np.float32), mm355.NV12, mm355.RGBA8),         # destination dtype
            (nv[:-1], rgba, mm355.NV12, mm355.RGBA8),                               # source rows
            (pw, rgba, mm355.NV12, mm355.RGBA8),                                    # words for a byte format
            (nv, rgba, mm355.P010, mm355.RGBA8),                                    # bytes for a word format
            (np.zeros((H * 3, W), np.uint8)[::2], rgba, mm355.NV12, mm355.RGBA8),   # a strided 4:2:0 frame
            (rgba, pw, None, mm355.NV12),                                           # destination dtype
            (rgba, nv[:, :-2], None, mm355.NV12),                                   # destination width
            (rgba, rgba.copy(), None, mm355.NV12),                                  # an RGBA8 frame for NV12
            (np.zeros((H, W, 4), np.float32), nv, None, mm355.NV12),                # RGBA32F in: no such pair
            (rgba, pw, None, mm355.P010),                                           # RGBA8 to P010: no such pair
            (nv, pw, mm355.NV12, mm355.P010),
            (nv, rgba, 20, mm355.RGBA8),                                            # an unknown code
        ]
        for src, dst, f, d in bad:
            with pytest.raises(mm355.MMError) as ei:
                proc.OnRenderImage(src, dst, fmt=f, dst_fmt=d)
            assert ei.value.code in (INVALID, UNSUPPORTED)
        assert _code(lambda: proc.OnRenderImage(rgba, pw, dst_fmt=mm355.P010)) == UNSUPPORTED
        assert _code(lambda: proc.OnRenderImage(nv, rgba, fmt=20, dst_fmt=mm355.RGBA8)) == INVALID
        assert len(rec.calls) == n                    # nothing reached the library
    finally:
        proc._handle = None


# ---- the plain conversion's numpy definitions, on pixels computed by hand ----

def _nv12(y, cb, cr):
    """A 2 x 2 NV12 frame: four luma codes, one (Cb, Cr) pair."""
    return np.array([[y[0], y[1]], [y[2], y[3]], [cb, cr]], np.uint8)


def test_neutral_chroma_decodes_to_gray():
    # limited range: (Y - 16) / 219 on all three channels; 16 -> 0, 235 -> 255, 126 -> 128.08 -> 128
    got = C.plain(_nv12((16, 235, 126, 125), 128, 128), mm355.NV12, mm355.RGBA8)
    want = [[0, 255], [128, 127]]                     # 125: 109 / 219 * 255 = 126.92 -> 127
    for c in range(3):
        assert got[..., c].tolist() == want
    assert (got[..., 3] == 255).all()
    # full range: the byte itself
    got = C.plain(_nv12((0, 255, 7, 200), 128, 128), mm355.NV12_FULL, mm355.RGBA8)
    assert got[..., 1].tolist() == [[0, 255], [7, 200]]
    # P010 words keep all 16 bits: 64 << 6 is black, 940 << 6 white; 10-bit code 502 is y = 1 / 2
    # exactly, 127.5 -> 128, and the word one sixty-fourth of a code below it (501 + 63 / 64:
    # 437.984 / 876 * 255 = 127.4955) rounds down, which a decode of the 10-bit code alone would miss
    w = np.array([[64 << 6, 940 << 6], [(501 << 6) + 63, 502 << 6], [512 << 6, 512 << 6]], np.uint16)
    got = C.plain(w, mm355.P010, mm355.RGBA8)
    assert got[..., 0].tolist() == [[0, 255], [127, 128]]


def test_out_of_gamut_values_saturate():
    # Cr at its maximum on mid gray: R = 0.5 + 1.402 * 0.5 > 1, G = 0.5 - 0.357 = 0.1429..., B = 0.5
    y = 16 + 219 // 2                                  # 125: y = 109 / 219
    got = C.plain(_nv12((y, y, y, y), 128, 240), mm355.NV12, mm355.RGBA8)
    yv = 109 / 219
    assert got[0, 0].tolist() == [255, int(np.floor((yv - 0.714136 * 0.5) * 255 + 0.5)), int(np.floor(yv * 255 + 0.5)), 255]
    # Cb at its minimum: B below zero
    got = C.plain(_nv12((y, y, y, y), 16, 128), mm355.NV12, mm355.RGBA8)
    assert got[0, 0, 2] == 0 and got[0, 0, 0] == int(np.floor(yv * 255 + 0.5))
    # BT.709: R = y + 1.5748 cr
    got = C.plain(_nv12((y, y, y, y), 128, 128 + 56), mm355.NV12 | mm355.MATRIX_BT709, mm355.RGBA8)
    assert got[0, 0, 0] == int(np.floor((yv + 1.5748 * 0.25) * 255 + 0.5))


def test_encode_takes_the_2x2_mean_and_ignores_alpha():
    # one red pixel in a black block: Y' = 0.299, Cb' = -0.299 / 1.772, Cr' = 0.701 / 1.402 = 0.5
    px = np.zeros((2, 2, 4), np.uint8)
    px[0, 0] = (255, 0, 0, 7)                          # (any alpha)
    got = C.plain(px, mm355.RGBA8, mm355.NV12)
    assert got[:2].tolist() == [[int(np.floor(16 + 0.299 * 219 + 0.5)), 16], [16, 16]]
    cb = 128 + 224 * (-0.299 * 0.5 / 0.886) / 4
    cr = 128 + 224 * 0.5 / 4
    assert got[2].tolist() == [int(np.floor(cb + 0.5)), int(np.floor(cr + 0.5))] == [119, 156]
    px[..., 3] = 255
    assert np.array_equal(C.plain(px, mm355.RGBA8, mm355.NV12), got)
    # full range and BT.709 use the OUT code's weights and scales
    got = C.plain(px, mm355.RGBA8, mm355.NV12_FULL | mm355.MATRIX_BT709)
    assert got[0, 0] == int(np.floor(0.2126 * 255 + 0.5)) and got[2, 1] == int(np.floor(128 + 255 * 0.5 / 4 + 0.5))
    # white stays white, neutral chroma exactly 128
    px[...] = 255
    assert C.plain(px, mm355.RGBA8, mm355.NV12).tolist() == [[235, 235], [235, 235], [128, 128]]


def test_rounding_at_one_half():
    # RGBA8 out: floor(v * 255 + 0.5); NV12_FULL luma 1 is v = 1 / 255 exactly -> 1, and full-range
    # gray bytes pass unchanged through decode and store
    ramp = np.arange(4, dtype=np.uint8)
    got = C.plain(_nv12(ramp * 85, 128, 128), mm355.NV12_FULL, mm355.RGBA8)
    assert got[..., 0].reshape(-1).tolist() == [0, 85, 170, 255]
    # NV12 out, gray v = byte / 255: the luma code 16 + 219 v; v = 35 / 255 gives 46.0588 -> 46 and
    # v = 128 / 255 gives 125.93 -> 126; a code that lands on .5 exactly rounds up: full range,
    # the chroma sum of two white-blue pixels, Cb' = 0.5 each, mean 0.25: 128 + 63.75 = 191.75 -> 192
    px = np.zeros((2, 2, 4), np.uint8)
    px[..., :3] = 35
    px[1, 1, :3] = 128
    got = C.plain(px, mm355.RGBA8, mm355.NV12)
    assert got[:2].tolist() == [[46, 46], [46, 126]]
    px[...] = 0
    px[0, :, 2] = 255                                  # two pure blue pixels
    got = C.plain(px, mm355.RGBA8, mm355.NV12_FULL)
    assert got[2, 0] == 192
    assert C.store(np.full((2, 2, 3), 0.5 / 255.0), mm355.RGBA8)[0, 0, 0] == 1      # .5 rounds up
    assert C.store(np.full((2, 2, 3), 1.5 / 255.0), mm355.RGBA8)[0, 0, 0] == 2
