"""MM_YUY2 / MM_UYVY (packed 8-bit 4:2:2) on the host (no GPU): the format
codes the C ABI accepts and refuses, sizes and surface rules, mm_ycbcr_matrix,
the Python layer's shapes, the Y4M module's C422 entry points, and the
test-side codec (tests/yuv422.py) pinned to tests/ycbcr.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mm355
import mmtest as T
import ycbcr
import yuv422

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phase-based-motion-manipulation_amd")
LIB = os.path.join(PKG, "lib", "liby4m.so")

BASES = (24, 25, 26, 27)
BITS = (32, 64)
MATRIXED = [b | m for m in BITS for b in BASES]
VALID = list(BASES) + MATRIXED
# everything the earlier host tests pin as invalid, the same combinations on the
# new codes, and the codes kept free for a 10-bit form
INVALID = ([4, 5, 6, 7, 12, 15, 20, 20 | 32, 32, 64, 28, 29, 30, 31] +
           [f | m for f in (0, 1, 2, 3, 8, 9, 10, 11) for m in BITS] +          # a matrix bit on an RGBA or Y code
           [b | 96 for b in BASES + (16, 18)] +                                  # both bits together
           [b | 128 for b in BASES] + [b | 128 | 32 for b in BASES] +            # bit 128
           [c | m for c in (28, 29, 30, 31) for m in BITS] + [-1, -24, 24 | 256])


class Info(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("fps_num", ctypes.c_int),
                ("fps_den", ctypes.c_int), ("aspect_num", ctypes.c_int),
                ("aspect_den", ctypes.c_int), ("chroma", ctypes.c_int), ("interlace", ctypes.c_char)]


@pytest.fixture(scope="module")
def y4m():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", PKG, "lib/liby4m.so"])
    L = ctypes.CDLL(LIB)
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.y4m_read_header.argtypes = [vp, ctypes.POINTER(Info)]
    L.y4m_read_header_depth.argtypes = [vp, ctypes.POINTER(Info), ctypes.POINTER(ci)]
    L.y4m_frame_bytes.restype = ctypes.c_size_t
    L.y4m_frame_bytes.argtypes = [ctypes.POINTER(Info)]
    L.y4m_read_frame.argtypes = [vp, ctypes.POINTER(Info), vp]
    L.y4m_422_to_packed.restype = None
    L.y4m_422_to_packed.argtypes = [ci, ci, vp, vp, ci]
    L.y4m_packed_to_422.restype = None
    L.y4m_packed_to_422.argtypes = [ci, ci, vp, vp, ci]
    L.y4m_write_header_422.argtypes = [vp, ci, ci, ci, ci]
    L.y4m_write_frame_422.argtypes = [vp, ci, ci, vp]
    return L, libc


def _code(call):
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def test_codes_and_header():
    assert (mm355.YUY2, mm355.YUY2_FULL, mm355.UYVY, mm355.UYVY_FULL) == BASES
    for name in ("YUY2", "YUY2_FULL", "UYVY", "UYVY_FULL"):
        assert name in mm355.__all__
        assert mm355.FORMAT_BPP[getattr(mm355, name)] == 2
    assert sorted(MATRIXED) == list(range(56, 60)) + list(range(88, 92))
    hdr = open(mm355.binding.HEADER).read()
    for name, code in (("MM_YUY2", 24), ("MM_YUY2_FULL", 25), ("MM_UYVY", 26), ("MM_UYVY_FULL", 27)):
        assert any(ln.split()[:3] == ["#define", name, str(code)] for ln in hdr.splitlines()), name
    assert "Packed 4:2:2 capture frames" in hdr
    assert mm355.lib().mm_abi_version() == 10
    assert [yuv422.fmt_code(m, f, u) for m in (601, 709, 2020) for u in (False, True) for f in (False, True)] == VALID
    for fmt in VALID:
        assert mm355.base_format(fmt) in BASES


@pytest.mark.parametrize("fmt", VALID)
def test_sizes_and_surfaces(fmt):
    assert mm355.frame_bytes(1920, 1080, fmt) == 4147200
    for W, H in ((1920, 1080), (98, 62), (64, 48), (2, 2)):
        assert mm355.frame_bytes(W, H, fmt) == 2 * W * H
        t = mm355.Surface.tight(W, H, fmt)
        assert (t.format, t.pitch, t.chroma_offset, t.chroma_pitch, t.frame_stride) == (fmt, 2 * W, 0, 0, 2 * W * H)
        assert t.bytes(W, H) == 2 * W * H
    # 1080p rows are 3,840 bytes, 15 x 256: aligned(256, 16) pads the rows only;
    # the next power of two up gives the 4,096-byte pitch
    a = mm355.Surface.aligned(1920, 1080, fmt, 256, 16)
    assert (a.pitch, a.chroma_offset, a.chroma_pitch, a.frame_stride) == (3840, 0, 0, 3840 * 1088)
    a = mm355.Surface.aligned(1920, 1080, fmt, 512, 16)
    assert (a.pitch, a.chroma_offset, a.chroma_pitch, a.frame_stride) == (4096, 0, 0, 4096 * 1088)
    assert a.bytes(1920, 1080) == 4096 * 1079 + 3840
    a = mm355.Surface.aligned(200, 120, fmt, 256, 16)
    assert (a.pitch, a.frame_stride) == (512, 512 * 128)
    # odd W or H: unsupported, not invalid
    for W, H in ((97, 63), (98, 63), (97, 62)):
        assert _code(lambda: mm355.frame_bytes(W, H, fmt)) == -2
        assert _code(lambda: mm355.Surface.tight(W, H, fmt)) == -2
        assert _code(lambda: mm355.Surface.aligned(W, H, fmt, 256, 16)) == -2
    # the unit is 4, one macropixel
    s = mm355.Surface.tight(64, 48, fmt)
    s.pitch += 4
    assert s.bytes(64, 48) == 132 * 47 + 128
    for bad in (2, 1, 3):
        s.pitch = 128 + 4 + bad
        assert _code(lambda: s.bytes(64, 48)) == -1
    s.pitch = 124                                        # shorter than a row
    assert _code(lambda: s.bytes(64, 48)) == -1
    for field in ("chroma_offset", "chroma_pitch"):
        s = mm355.Surface.tight(64, 48, fmt)
        setattr(s, field, 128 * 48 if field == "chroma_offset" else 128)
        assert _code(lambda: s.bytes(64, 48)) == -1
    assert _code(lambda: mm355.Surface.aligned(64, 48, fmt, 2, 1)) == -1      # pitch_align: a multiple of the unit
    assert mm355.Surface.aligned(64, 48, fmt, 4, 1).pitch == 128
    # a frame entry point refuses missing pointers
    assert mm355.lib().mm_process(None, None, None, fmt, 0, None) == -1


def test_mm_process_null_handle():
    assert mm355.lib().mm_process(None, None, None, mm355.YUY2, 0, None) == -1


@pytest.mark.parametrize("fmt", INVALID)
def test_invalid_codes_are_refused_before_unsupported(fmt):
    assert _code(lambda: mm355.frame_bytes(64, 48, fmt)) == -1
    assert _code(lambda: mm355.frame_bytes(97, 63, fmt)) == -1       # invalid before unsupported
    assert _code(lambda: mm355.Surface.tight(64, 48, fmt)) == -1
    assert _code(lambda: mm355.Surface.tight(97, 63, fmt)) == -1
    assert _code(lambda: mm355.Surface.aligned(64, 48, fmt, 256, 16)) == -1
    s = mm355.Surface.tight(64, 48, mm355.YUY2)
    s.format = fmt
    assert _code(lambda: s.bytes(64, 48)) == -1
    assert _code(lambda: mm355.ycbcr_matrix(fmt)) == -1
    assert mm355.lib().mm_process(None, None, None, fmt, 0, None) == -1


def test_ycbcr_matrix_is_the_420_codes():
    for bit in (0, 32, 64):
        want = mm355.ycbcr_matrix(mm355.NV12 | bit)
        for b in BASES:
            assert np.array_equal(mm355.ycbcr_matrix(b | bit), want)
    assert np.array_equal(mm355.ycbcr_matrix(mm355.YUY2 | mm355.MATRIX_BT709),
                          mm355.ycbcr_matrix(mm355.NV12 | mm355.MATRIX_BT709))
    m = mm355.ycbcr_matrix(mm355.UYVY_FULL)
    assert m[0, 0] == 0.0 and m[0, 1] == 0.0 and np.array_equal(m[1:], mm355.nv12_chroma_matrix())
    assert mm355.lib().mm_ycbcr_matrix(mm355.YUY2, None) == -1


def test_host_frames_and_layouts():
    for fmt in VALID:
        a = mm355.processor.host_frames(3, 48, 64, fmt)
        assert a.shape == (3, 48, 128) and a.dtype == np.uint8
        assert a.nbytes == 3 * mm355.frame_bytes(64, 48, fmt)
        assert mm355.frame_layout(a[0], 64, 48, fmt) is None                 # contiguous: the tight entry point
    parent = np.zeros((60, 2 * 80), np.uint8)
    lay = mm355.frame_layout(parent[6:54, 8:136], 64, 48, mm355.UYVY | mm355.MATRIX_BT709)
    assert (lay.format, lay.pitch, lay.chroma_offset, lay.chroma_pitch) == (mm355.UYVY | 32, 160, 0, 0)
    with pytest.raises(mm355.MMError):
        mm355.frame_layout(np.zeros((48, 64), np.uint8), 64, 48, mm355.YUY2)           # [H, W]: a Y8 frame's shape
    with pytest.raises(mm355.MMError):
        mm355.frame_layout(np.zeros((48, 128), np.uint16), 64, 48, mm355.YUY2)
    with pytest.raises(mm355.MMError):
        mm355.frame_layout(np.zeros((48, 256), np.uint8)[:, ::2], 64, 48, mm355.YUY2)   # bytes not packed
    with pytest.raises(mm355.MMError):
        mm355.frame_layout(np.zeros((48, 130), np.uint8)[:, :128], 64, 48, mm355.YUY2)  # pitch 130: no multiple of 4


def _read_header(y4m, path, depth_reader=True):
    L, libc = y4m
    info, depth = Info(), ctypes.c_int(-1)
    fp = libc.fopen(path.encode(), b"rb")
    rc = L.y4m_read_header_depth(fp, ctypes.byref(info), ctypes.byref(depth)) if depth_reader \
        else L.y4m_read_header(fp, ctypes.byref(info))
    return rc, info, depth.value, fp


def test_y4m_422_round_trip(y4m, tmp_path):
    L, libc = y4m
    W, H, n = 34, 26, 3
    rng = np.random.default_rng(422)
    planes = [rng.integers(0, 256, 2 * W * H, dtype=np.uint8) for _ in range(n)]
    path = str(tmp_path / "a.y4m")
    fp = libc.fopen(path.encode(), b"wb")
    assert L.y4m_write_header_422(fp, W, H, 60, 1) == 0
    for p in planes:
        assert L.y4m_write_frame_422(fp, W, H, p.ctypes.data) == 0
    libc.fclose(fp)
    raw = open(path, "rb").read()
    head, body = raw.split(b"\n", 1)
    assert head == f"YUV4MPEG2 W{W} H{H} F60:1 Ip A1:1 C422".encode()
    assert len(body) == n * (6 + 2 * W * H) and body[:6] == b"FRAME\n"
    rc, info, depth, fp = _read_header(y4m, path)
    assert rc == 0 and (info.width, info.height, info.chroma, depth, info.fps_num) == (W, H, 3, 8, 60)
    assert L.y4m_frame_bytes(ctypes.byref(info)) == 2 * W * H
    for p in planes:
        got = np.zeros(2 * W * H, np.uint8)
        assert L.y4m_read_frame(fp, ctypes.byref(info), got.ctypes.data) == 1
        assert np.array_equal(got, p)
        y, cb, cr = p[:W * H].reshape(H, W), p[W * H:W * H * 3 // 2].reshape(H, W // 2), p[W * H * 3 // 2:].reshape(H, W // 2)
        for uyvy in (0, 1):
            pk = np.full(2 * W * H, 0xA5, np.uint8)
            L.y4m_422_to_packed(W, H, p.ctypes.data, pk.ctypes.data, uyvy)
            assert np.array_equal(pk.reshape(H, 2 * W), yuv422.join(y, cb, cr, bool(uyvy)))
            back = np.full(2 * W * H, 0x5A, np.uint8)
            L.y4m_packed_to_422(W, H, pk.ctypes.data, back.ctypes.data, uyvy)
            assert np.array_equal(back, p)
    got = np.zeros(2 * W * H, np.uint8)
    assert L.y4m_read_frame(fp, ctypes.byref(info), got.ctypes.data) == 0       # end of stream
    libc.fclose(fp)
    # the plain reader keeps refusing the tag
    rc, _, _, fp = _read_header(y4m, path, depth_reader=False)
    libc.fclose(fp)
    assert rc == -1


def test_helper_round_trips_and_byte_orders():
    W, H = 64, 48
    rgb = T.synth(W, H, 1, fmt="u8")[0]
    flat = np.repeat(rgb[:, ::2], 2, 1)                     # constant over every macropixel
    for matrix in ycbcr.MATRICES:
        for full in (False, True):
            a = yuv422.encode(flat, matrix, full, False)
            b = yuv422.encode(flat, matrix, full, True)
            assert np.array_equal(yuv422.swap_order(a), b) and np.array_equal(yuv422.swap_order(b), a)
            for uyvy, x in ((False, a), (True, b)):
                d = yuv422.decode(x, np.float64, matrix, full, uyvy)
                assert np.array_equal(yuv422.encode(d, matrix, full, uyvy), x), (matrix, full, uyvy)   # stable
                assert np.array_equal(d, yuv422.decode(yuv422.swap_order(x), np.float64, matrix, full, not uyvy))
            g = a.copy()
            g[:, 1::2] = 128                                 # neutral chroma: R = G = B = y
            d = yuv422.decode(g, np.float64, matrix, full)
            assert np.array_equal(d[..., 0], d[..., 1]) and np.array_equal(d[..., 1], d[..., 2])
            assert np.all(d[..., 3] == 1.0)
    # hand values: limited-range black, white and a saturated blue-ish macropixel
    m = np.array([[16, 128, 235, 128]], np.uint8)
    d = yuv422.decode(m, np.float64)
    assert np.array_equal(d[0, :, :3], [[0, 0, 0], [1, 1, 1]])
    d = yuv422.decode(np.array([[41, 240, 41, 110]], np.uint8), np.float64)
    assert abs(d[0, 0, 2] - ((41 - 16) / 219 + 1.772 * 112 / 224)) < 1e-15 and np.array_equal(d[0, 0], d[0, 1])
    assert np.array_equal(yuv422.decode(np.array([[128, 16, 128, 235]], np.uint8), np.float64, uyvy=True)[0, :, :3],
                          [[0, 0, 0], [1, 1, 1]])
    s = yuv422.chroma_stress(yuv422.encode(rgb), 1)
    _, cb, cr = yuv422.split(s)
    assert cb.min() == 16 and cb.max() == 240 and cr.min() == 16 and cr.max() == 240
    assert np.array_equal(yuv422.split(s)[0], yuv422.split(yuv422.encode(rgb))[0])


def test_helper_agrees_with_ycbcr_on_2x2_constant_chroma():
    """BT.601 (and the matrixed) values are tests/ycbcr.py's on a frame whose
    2 x 2 chroma blocks are constant: the same decode pixel for pixel, and the
    same codes back (the 1 x 2 mean of two equal rows is the 2 x 2 mean)."""
    W, H = 70, 46
    rng = np.random.default_rng(601)
    for matrix in ycbcr.MATRICES:
        for full in (False, True):
            nv = rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
            c = nv[H:].reshape(H // 2, W // 2, 2)
            for uyvy in (False, True):
                buf = yuv422.join(nv[:H], np.repeat(c[..., 0], 2, 0), np.repeat(c[..., 1], 2, 0), uyvy)
                for dt in (np.float32, np.float64):
                    assert np.array_equal(yuv422.decode(buf, dt, matrix, full, uyvy),
                                          ycbcr.decode(nv, dt, matrix, full, 8))
            rgb = ycbcr.decode(nv, np.float64, matrix, full, 8)
            blocks = np.repeat(np.repeat(rgb[::2, ::2], 2, 0), 2, 1)     # constant 2 x 2 blocks, out of gamut too
            e420 = ycbcr.encode(blocks, matrix, full, 8)
            y, cb, cr = yuv422.split(yuv422.encode(blocks, matrix, full))
            assert np.array_equal(y, e420[:H])
            assert np.array_equal(cb[::2], e420[H:, 0::2]) and np.array_equal(cb[1::2], e420[H:, 0::2])
            assert np.array_equal(cr[::2], e420[H:, 1::2]) and np.array_equal(cr[1::2], e420[H:, 1::2])


def _clip(path, tag, W=16, H=16, nbytes=None):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C{tag}\n".encode())
        f.write(b"FRAME\n" + bytes(nbytes if nbytes is not None else 2 * W * H))


def test_cli_refusals(tmp_path):
    """Refused combinations end with the usage status (2) and a message that
    names the option, before any device is touched."""
    cli = os.path.join(PKG, "bin", "mm_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", PKG])
    c422, c420, odd, m8 = (str(tmp_path / n) for n in ("c422.y4m", "c420.y4m", "odd.y4m", "m8.y4m"))
    _clip(c422, "422")
    _clip(c420, "420", nbytes=16 * 16 * 3 // 2)
    _clip(odd, "422", W=16, H=15)
    _clip(m8, "mono", nbytes=16 * 16)
    out = str(tmp_path / "out.y4m")
    ring = ["--ring-world", "2", "--ring-rank", "0", "--ring-id", str(tmp_path / "id")]
    for opt in ("--yuy2", "--uyvy"):
        cases = [[opt, "-i", c422, "--srgb"], [opt, "-i", c422, "--show-magnitude"], [opt, "-i", c422, "--show-phase"],
                 [opt, "-i", c422, "--ring-local", "2"], [opt, "-i", c422] + ring,
                 [opt, "-i", c422, "--nv12"], [opt, "-i", c422, "--p010"], [opt, "-i", c422, "--mono"],
                 [opt, "-i", c420], [opt, "-i", m8], [opt], [opt, "-w", "16", "-h", "16"],   # not a C422 input
                 [opt, "-i", odd]]                                                           # odd height
        for args in cases:
            r = subprocess.run([cli] + args + ["-o", out, "-n", "1"], capture_output=True, timeout=60)
            assert r.returncode == 2, (args, r.returncode, r.stderr)
            assert opt.encode() in r.stderr, (args, r.stderr)
    r = subprocess.run([cli, "--yuy2", "--uyvy", "-i", c422, "-o", out], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--yuy2" in r.stderr and b"--uyvy" in r.stderr
    # a C422 clip without either flag: never converted on the host
    for extra in ([], ["--srgb"], ["--full-range"]):
        r = subprocess.run([cli, "-i", c422, "-o", out, "-n", "1"] + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--yuy2" in r.stderr and b"--uyvy" in r.stderr, (extra, r.stderr)
    # --matrix keeps its usage errors, and now goes with these flags
    for args in (["--matrix", "709", "-i", c420], ["--yuy2", "--matrix", "240", "-i", c422]):
        r = subprocess.run([cli] + args + ["-o", out, "-n", "1"], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--matrix" in r.stderr, (args, r.stderr)
