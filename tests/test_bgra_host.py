"""MM_BGRA8 / MM_BGRA8_SRGB on the host: the codes, their sizes and layouts (which
are MM_RGBA8's), the refusal list, mm_convert_supported's table with the two new
codes, OnRenderImage's shape and dtype checks and the CLI's usage errors.  None
of it touches a GPU.  Every test fails on a library from before the formats,
where 8192 is MM_ERR_INVALID (the fixture below asks first)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mm355
from mm355 import Surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phase-based-motion-manipulation_amd")
CLI = os.path.join(PKG, "bin", "mm_cli")
OK, INVALID, UNSUPPORTED = 0, -1, -2
BGRA8, BGRA8_SRGB = 8192, 8195
PAIRS = ((BGRA8, mm355.RGBA8), (BGRA8_SRGB, mm355.RGBA8_SRGB))
SIZES = ((2, 2), (97, 63), (98, 62), (1920, 1080), (8192, 8192))
NV12_CODES = (16, 17, 48, 49, 80, 81)
P010_CODES = (18, 19, 50, 51, 82, 83)

with open(os.path.join(ROOT, "tests", "golden", "format_table.json")) as _f:
    GOLD = json.load(_f)
# every code valid before the BGRA formats: the fixture's, and v210's six (added after it was recorded)
OLD_VALID = tuple(GOLD["valid_codes"]) + (4118, 4119, 4150, 4151, 4182, 4183)

# the refusal list of include/mm.h "BGRA frames", code by code
BAD_CODES = (
    128, 131,                                   # MM_ORDER_BGR on the RGBA8 codes stays no format
    8193, 8194,                                 # float BGRA
    8192 | 8, 8192 | 11, 8192 | 13, 8192 | 141,             # single-plane, packed RGB
    8192 | 16, 8192 | 17, 8192 | 18, 8192 | 22, 8192 | 24, 8192 | 26,   # Y'CbCr
    8192 | 528, 8192 | 1554, 8192 | 4118,       # planar, low-bits, v210
    22 | 8192, 22 | 4096 | 8192,
    8192 | 32, 8192 | 64, 8195 | 32,            # a matrix bit
    8192 | 128, 8195 | 128,                     # both order bits
    8192 | 256, 8192 | 512, 8192 | 1024, 8192 | 4096, 8195 | 4096,
    16384, 16384 | 8192, 16384 | 8195, 32768 | 8192, 1 << 30 | 8192,
    -8192, -8195,
)


@pytest.fixture(autouse=True)
def _the_formats_exist():
    """include/mm.h's detection: mm_frame_bytes(W, H, MM_BGRA8, &n) == MM_OK."""
    n = ctypes.c_size_t()
    assert mm355.lib().mm_frame_bytes(2, 2, BGRA8, ctypes.byref(n)) == OK and n.value == 16


def _code(call):
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def test_constants_and_detection():
    assert mm355.ORDER_BGRA == 8192 and mm355.BGRA8 == BGRA8 and mm355.BGRA8_SRGB == BGRA8_SRGB
    assert mm355.BGRA_FORMATS == (BGRA8, BGRA8_SRGB)
    assert mm355.FORMAT_BPP[BGRA8] == 4 and mm355.FORMAT_BPP[BGRA8_SRGB] == 4
    assert mm355.base_format(BGRA8) == BGRA8 and mm355.row_bytes(97, BGRA8) == 388
    assert mm355.has_bgra()
    assert mm355.lib().mm_abi_version() == 10             # a backward-compatible addition
    hdr = open(mm355.binding.HEADER).read()
    for line in ("#define MM_ORDER_BGRA 8192", "#define MM_BGRA8      (MM_RGBA8 | MM_ORDER_BGRA)",
                 "#define MM_BGRA8_SRGB (MM_RGBA8_SRGB | MM_ORDER_BGRA)"):
        assert line in hdr, line


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fmt,twin", PAIRS)
def test_sizes_and_layouts_are_rgba8s(fmt, twin, W, H):
    assert mm355.frame_bytes(W, H, fmt) == mm355.frame_bytes(W, H, twin) == 4 * W * H
    a, b = Surface.tight(W, H, fmt), Surface.tight(W, H, twin)
    assert a.format == fmt
    assert (a.pitch, a.chroma_offset, a.chroma_pitch, a.frame_stride) == \
           (b.pitch, b.chroma_offset, b.chroma_pitch, b.frame_stride) == (4 * W, 0, 0, 4 * W * H)
    assert a.bytes(W, H) == b.bytes(W, H) == 4 * W * H
    for pa, ra in ((256, 16), (4, 1), (64, 2)):
        a, b = Surface.aligned(W, H, fmt, pa, ra), Surface.aligned(W, H, twin, pa, ra)
        assert a.format == fmt
        assert (a.pitch, a.chroma_offset, a.chroma_pitch, a.frame_stride) == \
               (b.pitch, b.chroma_offset, b.chroma_pitch, b.frame_stride)
        assert a.bytes(W, H) == b.bytes(W, H) == a.pitch * (H - 1) + 4 * W
    assert _code(lambda: Surface.aligned(W, H, fmt, 6, 1)) == INVALID      # a pitch alignment off the unit


def test_the_header_s_surface_examples():
    s = Surface.aligned(1920, 1080, BGRA8, 256, 16)
    assert (s.pitch, s.frame_stride) == (7680, 8355840)
    s = Surface.aligned(97, 63, BGRA8, 256, 16)
    assert (s.pitch, s.frame_stride) == (512, 32768)


@pytest.mark.parametrize("fmt", (BGRA8, BGRA8_SRGB))
def test_unit_is_four_and_there_is_no_chroma_plane(fmt):
    W, H = 98, 62
    s = Surface.tight(W, H, fmt)
    s.pitch = 4 * W + 4
    assert s.bytes(W, H) == (4 * W + 4) * (H - 1) + 4 * W
    for pitch in (4 * W + 2, 4 * W + 1, 4 * W - 4):        # 2 mod 4, odd, shorter than a row
        s.pitch = pitch
        assert _code(lambda: s.bytes(W, H)) == INVALID, pitch
    for field in ("chroma_offset", "chroma_pitch"):
        s = Surface.tight(W, H, fmt)
        setattr(s, field, 4 * W * H)
        assert _code(lambda: s.bytes(W, H)) == INVALID, field
    # (a device base at 2 mod 4 is refused by the frame entry points, which need a
    # handle: test_bgra.py::test_refusals_leave_the_next_output_unchanged)


@pytest.mark.parametrize("bad", BAD_CODES)
def test_refusal_list(bad):
    lib = mm355.lib()
    n = ctypes.c_size_t(7)
    s = Surface()
    assert lib.mm_frame_bytes(64, 48, bad, ctypes.byref(n)) == INVALID and n.value == 7
    assert lib.mm_surface_tight(64, 48, bad, ctypes.byref(s)) == INVALID
    assert lib.mm_surface_aligned(64, 48, bad, 256, 16, ctypes.byref(s)) == INVALID
    s = Surface(format=bad, pitch=256, chroma_offset=0, chroma_pitch=0, frame_stride=256 * 48)
    assert lib.mm_surface_bytes(64, 48, ctypes.byref(s), ctypes.byref(n)) == INVALID
    assert mm355.convert_supported(bad, bad) == INVALID
    assert mm355.convert_supported(bad, mm355.NV12) == INVALID
    assert mm355.convert_supported(mm355.NV12, bad) == INVALID


def test_convert_table():
    codes = OLD_VALID + (BGRA8, BGRA8_SRGB)
    for c in NV12_CODES + P010_CODES:
        assert mm355.convert_supported(c, BGRA8) == OK, c               # decode
    for c in NV12_CODES:
        assert mm355.convert_supported(BGRA8, c) == OK, c               # encode
    for a in codes:
        for b in codes:
            got = mm355.convert_supported(a, b)
            if a == b:
                assert got == OK, (a, b)
            elif BGRA8 in (a, b) or BGRA8_SRGB in (a, b):
                new = (a in NV12_CODES + P010_CODES and b == BGRA8) or (a == BGRA8 and b in NV12_CODES)
                assert got == (OK if new else UNSUPPORTED), (a, b)
    # the answers among the old codes are the golden fixture's
    sides = GOLD["convert_sides"]
    for a in sides:
        for j, b in enumerate(sides):
            assert mm355.convert_supported(a, b) == GOLD["convert"][str(a)][j], (a, b)
    # RGBA8 <-> BGRA8 is no pair, nor is anything with the sRGB code
    for a, b in ((0, BGRA8), (BGRA8, 0), (3, BGRA8_SRGB), (BGRA8_SRGB, 3), (BGRA8, BGRA8_SRGB),
                 (16, BGRA8_SRGB), (BGRA8_SRGB, 16), (BGRA8, 18), (13, BGRA8), (BGRA8, 141), (528, BGRA8),
                 (BGRA8, 528), (24, BGRA8), (4118, BGRA8)):
        assert mm355.convert_supported(a, b) == UNSUPPORTED, (a, b)


def test_no_matrix():
    m = (ctypes.c_double * 6)()
    for c in (BGRA8, BGRA8_SRGB):
        assert mm355.lib().mm_ycbcr_matrix(c, m) == INVALID


class _Recorder:
    """Stands in for the handle: records what OnRenderImage would call
    (tests/test_convert_host.py's double)."""

    def __init__(self):
        self.calls = []

    def process(self, *a, **kw):
        self.calls.append(("process", a, kw))

    def process_surface(self, *a, **kw):
        self.calls.append(("process_surface", a, kw))

    def process_convert(self, *a, **kw):
        self.calls.append(("process_convert", a, kw))


def test_on_render_image_shapes_and_dtypes():
    W, H = 64, 48
    proc = mm355.MotionMagnificationProcessor(W, H)
    proc._handle = rec = _Recorder()
    px = np.zeros((H, W, 4), np.uint8)
    nv = np.zeros((H * 3 // 2, W), np.uint8)
    pw = np.zeros((H * 3 // 2, W), np.uint16)
    try:
        for fmt in (mm355.BGRA8, mm355.BGRA8_SRGB):
            proc.OnRenderImage(px, px.copy(), fmt=fmt)
            name, a, kw = rec.calls[-1]
            assert name == "process" and a[2] == fmt and kw["on_device"] is False
        # a region of interest keeps its own layout, with the BGRA code
        parent = np.zeros((100, 90, 4), np.uint8)
        proc.OnRenderImage(parent[7:7 + H, 5:5 + W], px.copy(), fmt=mm355.BGRA8)
        name, a, kw = rec.calls[-1]
        assert name == "process_surface" and (a[1].format, a[1].pitch) == (BGRA8, 360)
        assert (a[3].format, a[3].pitch) == (BGRA8, 4 * W)
        # the pairs: each side by its own format
        proc.OnRenderImage(nv, px.copy(), fmt=mm355.NV12 | mm355.MATRIX_BT709, dst_fmt=mm355.BGRA8)
        name, a, kw = rec.calls[-1]
        assert name == "process_convert" and (a[1].format, a[3].format, a[3].pitch) == (48, BGRA8, 4 * W)
        proc.OnRenderImage(pw, px.copy(), fmt=mm355.P010, dst_fmt=mm355.BGRA8)
        assert rec.calls[-1][0] == "process_convert"
        proc.OnRenderImage(px, nv.copy(), fmt=mm355.BGRA8, dst_fmt=mm355.NV12_FULL)
        name, a, kw = rec.calls[-1]
        assert name == "process_convert" and (a[1].format, a[3].format) == (BGRA8, 17)
        proc.OnRenderImage(px, px.copy(), fmt=mm355.BGRA8, dst_fmt=mm355.BGRA8)
        assert rec.calls[-1][0] == "process"
        n = len(rec.calls)
        bad = [
            (np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8), mm355.BGRA8, None),    # three channels
            (np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), mm355.BGRA8, None),          # no channels
            (px[:-1], px[:-1].copy(), mm355.BGRA8, None),                                         # rows
            (px, px[:, :-1].copy(), mm355.BGRA8, None),                                           # destination width
            (np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), mm355.BGRA8, None),   # no float BGRA
            (np.zeros((H, W, 4), np.float16), np.zeros((H, W, 4), np.float16), mm355.BGRA8_SRGB, None),
            (px, np.zeros((H, W, 4), np.uint16), mm355.BGRA8, None),                              # destination dtype
            (np.zeros((H, W, 8), np.uint8)[:, :, ::2], px.copy(), mm355.BGRA8, None),             # channels not packed
            (np.zeros((H, 2 * W, 4), np.uint8)[:, ::2], px.copy(), mm355.BGRA8, None),            # pixels not packed
            (nv, np.zeros((H, W, 3), np.uint8), mm355.NV12, mm355.BGRA8),                         # pair: destination shape
            (nv, np.zeros((H, W, 4), np.float32), mm355.NV12, mm355.BGRA8),                       # ... dtype
            (px, pw, mm355.BGRA8, mm355.NV12),                                                    # words for NV12
            (px, pw, mm355.BGRA8, mm355.P010),                                                    # no P010 out
            (px, px.copy(), mm355.BGRA8, mm355.RGBA8),                                            # no swizzle transcode
            (px, px.copy(), None, mm355.BGRA8),
            (nv, px.copy(), mm355.NV12, mm355.BGRA8_SRGB),                                        # the sRGB code has no pair
            (px, px.copy(), 8193, None),                                                          # an unknown code
        ]
        for src, dst, f, d in bad:
            with pytest.raises(mm355.MMError) as ei:
                proc.OnRenderImage(src, dst, fmt=f, dst_fmt=d)
            assert ei.value.code in (INVALID, UNSUPPORTED), (src.shape, f, d)
        assert _code(lambda: proc.OnRenderImage(px, px.copy(), fmt=mm355.BGRA8, dst_fmt=mm355.RGBA8)) == UNSUPPORTED
        assert len(rec.calls) == n                    # nothing reached the library
    finally:
        proc._handle = None


def test_cli_usage_errors(tmp_path):
    """--bgra without --ppm, or with --bgr, ends with the usage status (2) before
    any file is written or any device touched."""
    src, out = str(tmp_path / "in.ppm"), str(tmp_path / "out.ppm")
    with open(src, "wb") as f:
        f.write(b"P6\n16 16\n255\n" + bytes(16 * 16 * 3))
    for args, word in ((["--bgra"], b"--ppm"), (["--bgra", "-i", src], b"--ppm"),
                       (["--ppm", "--bgra", "--bgr", "-i", src], b"--bgr"),
                       (["--ppm", "--bgr", "--bgra", "-i", src], b"--bgr"),
                       (["--out-bgra8"], b"--nv12"), (["--ppm", "-i", src, "--out-bgra8"], b"--out-bgra8"),
                       (["--out-bgra8", "--out-rgba8", "--nv12", "-i", src], b"--out-bgra8")):
        r = subprocess.run([CLI] + args + ["-o", out, "-n", "1"], capture_output=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert b"--bgra" in r.stderr or b"--out-bgra8" in r.stderr, (args, r.stderr)
        assert word in r.stderr, (args, r.stderr)
        assert not os.path.exists(out), args
