"""MM_NV12 / MM_NV12_FULL on the host (no GPU): the format codes and sizes in
the C ABI, the Y4M module's NV12 helpers and C420 writer, and the test-side
codec (tests/nv12.py) pinned to the project's existing BT.601 conversion."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mm355
import nv12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phase-based-motion-manipulation_amd")
LIB = os.path.join(PKG, "lib", "liby4m.so")


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
    L.y4m_frame_bytes.restype = ctypes.c_size_t
    L.y4m_frame_bytes.argtypes = [ctypes.POINTER(Info)]
    L.y4m_read_frame.argtypes = [vp, ctypes.POINTER(Info), vp]
    L.y4m_to_rgba.argtypes = [ctypes.POINTER(Info), vp, vp, ci]
    L.y4m_420_to_nv12.argtypes = [ci, ci, vp, vp]
    L.y4m_nv12_to_420.argtypes = [ci, ci, vp, vp]
    L.y4m_write_header_420.argtypes = [vp, ci, ci, ci, ci]
    L.y4m_write_frame_420.argtypes = [vp, ci, ci, vp]
    return L, libc


def test_format_codes_and_frame_bytes():
    assert (mm355.NV12, mm355.NV12_FULL) == (16, 17)
    assert "NV12" in mm355.__all__ and "NV12_FULL" in mm355.__all__
    assert mm355.frame_bytes(1920, 1080, mm355.NV12) == 3110400
    assert mm355.frame_bytes(1920, 1080, mm355.NV12_FULL) == 3110400
    assert mm355.frame_bytes(98, 62, mm355.NV12) == 9114
    for W, H in ((97, 63), (98, 63), (97, 62)):
        with pytest.raises(mm355.MMError) as ei:
            mm355.frame_bytes(W, H, mm355.NV12)
        assert ei.value.code == -2                       # MM_ERR_UNSUPPORTED
    with pytest.raises(mm355.MMError) as ei:
        mm355.frame_bytes(64, 48, 4)                     # the codes start at 16
    assert ei.value.code == -1
    hdr = open(mm355.binding.HEADER).read()
    assert "#define MM_NV12      16" in hdr and "#define MM_NV12_FULL 17" in hdr
    assert mm355.lib().mm_abi_version() == 10
    # the frame entry points refuse an unknown code before they look at the handle's frames
    assert mm355.lib().mm_process(None, None, None, mm355.NV12, 0, None) == -1
    assert mm355.processor.host_frames(2, 48, 64, mm355.NV12).shape == (2, 72, 64)
    assert mm355.processor.host_frames(2, 48, 64, mm355.NV12_FULL).dtype == np.uint8


def test_y4m_nv12_round_trip_and_c420_writer(y4m, tmp_path):
    L, libc = y4m
    W, H, n = 70, 46, 3
    rng = np.random.default_rng(12)
    planes = [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8) for _ in range(n)]
    path = str(tmp_path / "c420.y4m")
    fp = libc.fopen(path.encode(), b"wb")
    assert L.y4m_write_header_420(fp, W, H, 30000, 1001) == 0
    for p in planes:
        nv = np.zeros(W * H * 3 // 2, np.uint8)
        L.y4m_420_to_nv12(W, H, p.ctypes.data, nv.ctypes.data)
        # interleaved with no arithmetic: Y kept, (Cb, Cr) pairs in plane order
        assert np.array_equal(nv[:W * H], p[:W * H])
        c = nv[W * H:].reshape(-1, 2)
        assert np.array_equal(c[:, 0], p[W * H:W * H * 5 // 4])
        assert np.array_equal(c[:, 1], p[W * H * 5 // 4:])
        back = np.zeros_like(p)
        L.y4m_nv12_to_420(W, H, nv.ctypes.data, back.ctypes.data)
        assert np.array_equal(back, p)
        assert L.y4m_write_frame_420(fp, W, H, back.ctypes.data) == 0
    libc.fclose(fp)
    # the file reads back through the existing reader
    fp = libc.fopen(path.encode(), b"rb")
    info = Info()
    assert L.y4m_read_header(fp, ctypes.byref(info)) == 0
    assert (info.width, info.height, info.chroma, info.fps_num, info.fps_den) == (W, H, 0, 30000, 1001)
    assert L.y4m_frame_bytes(ctypes.byref(info)) == W * H * 3 // 2
    for p in planes:
        buf = np.zeros(W * H * 3 // 2, np.uint8)
        assert L.y4m_read_frame(fp, ctypes.byref(info), buf.ctypes.data) == 1
        assert np.array_equal(buf, p)
    assert L.y4m_read_frame(fp, ctypes.byref(info), buf.ctypes.data) == 0
    libc.fclose(fp)


@pytest.mark.parametrize("full", [0, 1])
def test_codec_decode_agrees_with_y4m_to_rgba(y4m, full):
    """decode() is y4m_to_rgba before its byte rounding: on in-gamut input the
    bytes y4m_to_rgba writes are round(255 decode()) up to its fp32 arithmetic
    (a value within 1e-3 of a rounding boundary may land on either side)."""
    import mmtest as T
    L, _ = y4m
    W, H = 64, 48
    for t, rgb in enumerate(T.synth(W, H, 3, fmt="u8")):
        buf = nv12.encode(rgb, full=bool(full))
        planes = np.zeros(W * H * 3 // 2, np.uint8)
        L.y4m_nv12_to_420(W, H, buf.ctypes.data, planes.ctypes.data)
        info = Info(W, H, 25, 1, 1, 1, 0, b"p")
        rgba = np.zeros((H, W, 4), np.uint8)
        L.y4m_to_rgba(ctypes.byref(info), planes.ctypes.data, rgba.ctypes.data, full)
        dec = nv12.decode(buf, np.float64, full=bool(full)) * 255.0
        ok = (dec[..., :3] > 0.0) & (dec[..., :3] < 255.0)        # in gamut: no clamp in either
        assert ok.mean() > 0.9
        d = np.abs(rgba[..., :3].astype(np.float64) - dec[..., :3])
        assert d[ok].max() <= 0.5 + 1e-3, d[ok].max()
        assert np.all(rgba[..., 3] == 255) and np.all(dec[..., 3] == 255.0)
        # and the codec round-trips its own output: encode(decode(x)) == x where in gamut everywhere
        if t == 0:
            gray = np.full((H, W, 3), 0.5)
            g = nv12.encode(gray, full=bool(full))
            assert np.array_equal(nv12.encode(nv12.decode(g, np.float64, bool(full)), bool(full)), g)
            assert np.all(g[H:] == 128)


def test_codec_chroma_stress_range():
    buf = nv12.chroma_stress(nv12.encode(np.full((120, 200, 3), 0.5)), 1)
    c = buf[120:]
    assert c.min() == 16 and c.max() == 240
    rgb = nv12.decode(buf, np.float64)[..., :3]
    # mid-gray luma: B = 0.5 -+ 1.772 * 0.5; far out of gamut, not clamped
    assert rgb.min() < -0.35 and rgb.max() > 1.35


def test_host_chroma_matrix():
    """The matrix the library derives for the NV12 compose is RGBToYIQ x BT.601."""
    m = mm355.nv12_chroma_matrix()
    assert np.abs(m - nv12.matrix_iq()).max() <= 1e-7
    # and the luma row of that product is (1, 0, 0): luma of the decoded pixel is y
    y = np.array([0.299, 0.587, 0.114])
    rgb = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]])
    assert np.abs(y @ rgb - [1.0, 0.0, 0.0]).max() < 2e-7
