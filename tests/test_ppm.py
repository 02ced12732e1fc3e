"""The C driver's binary PPM module (host/ppm.c, lib/libppm.so) on the CPU: every
header variant it accepts, every refusal with its own status, the stream reader
and the writer.  Plain ctypes; no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phase-based-motion-manipulation_amd")
LIB = os.path.join(PKG, "lib", "libppm.so")
OK, EOF, MAGIC, HEADER, MAXVAL, TRUNCATED, SIZE, ARG = 0, 1, -1, -2, -3, -4, -5, -6


class Info(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int)]


@pytest.fixture(scope="module")
def ppm():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", PKG, "lib/libppm.so"])
    L = ctypes.CDLL(LIB)
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.ppm_read_header.argtypes = [vp, ctypes.POINTER(Info)]
    L.ppm_read_pixels.argtypes = [vp, ctypes.POINTER(Info), vp]
    L.ppm_read_next.argtypes = [vp, ctypes.POINTER(Info), vp]
    L.ppm_write_frame.argtypes = [vp, ci, ci, vp]
    L.ppm_swap_rb.argtypes = [vp, ctypes.c_size_t]
    L.ppm_swap_rb.restype = None
    return L, libc


def _header_status(ppm, tmp_path, data):
    """(status, width, height, the byte the stream stands at) of one header."""
    L, libc = ppm
    path = str(tmp_path / "h.ppm")
    with open(path, "wb") as f:
        f.write(data)
    fp = libc.fopen(path.encode(), b"rb")
    pi = Info(-7, -7)
    rc = L.ppm_read_header(fp, ctypes.byref(pi))
    nxt = np.zeros(1, np.uint8)
    libc.fread.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    libc.fread.restype = ctypes.c_size_t
    got = libc.fread(nxt.ctypes.data, 1, 1, fp)
    libc.fclose(fp)
    return rc, pi.width, pi.height, (int(nxt[0]) if got else None)


HEADERS_OK = [
    b"P6\n4 3\n255\n",                       # what ffmpeg and the writer emit
    b"P6 4 3 255 ",                          # single spaces
    b"P6\t4\r\n3\v\f255\t",                  # any whitespace, runs of it
    b"P6\n# made by a test\n4 3\n255\n",     # a comment line
    b"P6\n4 # width\n3 # height\n255\n",     # comments after fields
    b"P6\n4#w\n3\n#\n# two\n255\n",          # a comment right behind a number, an empty one
    b"P6#c\n4 3 255\n",                      # ... and right behind the magic
    b"P6\n004 03\n255\n",                    # leading zeros
]


@pytest.mark.parametrize("head", HEADERS_OK)
def test_header_variants(ppm, tmp_path, head):
    rc, w, h, nxt = _header_status(ppm, tmp_path, head + b"\x2a" + bytes(35))
    assert (rc, w, h) == (OK, 4, 3), head
    assert nxt == 0x2a, "exactly one whitespace byte separates maxval from the pixels"


def test_a_pixel_byte_that_is_whitespace_or_hash_is_data(ppm, tmp_path):
    for first in (b"\n", b" ", b"#"):
        rc, w, h, nxt = _header_status(ppm, tmp_path, b"P6\n2 1\n255\n" + first + bytes(5))
        assert (rc, w, h, nxt) == (OK, 2, 1, first[0])


REFUSALS = [
    (b"P3\n2 1\n255\n0 0 0 0 0 0\n", MAGIC),           # text PPM
    (b"P5\n2 1\n255\n\0\0", MAGIC),                     # binary gray
    (b"p6\n2 1\n255\n" + bytes(6), MAGIC),
    (b"YUV4MPEG2 W2 H1\n", MAGIC),
    (b"P", MAGIC),
    (b"P6\n2 1\n65535\n" + bytes(12), MAXVAL),          # 16-bit PPM
    (b"P6\n2 1\n254\n" + bytes(6), MAXVAL),
    (b"P6\n2 1\n1\n" + bytes(6), MAXVAL),
    (b"P65 4 255\n", HEADER),                           # the magic must end
    (b"P6\n2 x\n255\n", HEADER),
    (b"P6\n2x1\n255\n", HEADER),
    (b"P6\n-2 1\n255\n", HEADER),
    (b"P6\n0 1\n255\n", HEADER),
    (b"P6\n2 0\n255\n", HEADER),
    (b"P6\n99999999999 1\n255\n", HEADER),              # no overflow: a bound
    (b"P6\n2 1\n", HEADER),                             # ends inside the header
    (b"P6\n2 1\n255", HEADER),                          # no separator byte
    (b"P6\n2 1\n255x", HEADER),
    (b"P6\n2 1\n# never ends", HEADER),
    (b"P6", HEADER),
    (b"", EOF),                                         # a clean end
]


@pytest.mark.parametrize("data,want", REFUSALS)
def test_header_refusals_have_distinct_statuses(ppm, tmp_path, data, want):
    rc, w, h, _ = _header_status(ppm, tmp_path, data)
    assert rc == want, (data, rc)
    if rc != OK:
        assert (w, h) == (-7, -7), "a refused header leaves the caller's struct alone"
    assert len({OK, EOF, MAGIC, HEADER, MAXVAL, TRUNCATED, SIZE, ARG}) == 8


def _stream(frames):
    return b"".join(f"P6\n{f.shape[1]} {f.shape[0]}\n255\n".encode() + f.tobytes() for f in frames)


def _read_all(ppm, path, cap=16):
    """(frames, final status) of a stream, read as mm_cli reads it."""
    L, libc = ppm
    fp = libc.fopen(path.encode(), b"rb")
    first = Info()
    rc = L.ppm_read_header(fp, ctypes.byref(first))
    out = []
    if rc == OK:
        buf = np.zeros((first.height, first.width, 3), np.uint8)
        rc = L.ppm_read_pixels(fp, ctypes.byref(first), buf.ctypes.data)
        while rc == OK and len(out) < cap:
            out.append(buf.copy())
            rc = L.ppm_read_next(fp, ctypes.byref(first), buf.ctypes.data)
    libc.fclose(fp)
    return out, rc


def test_stream_round_trip(ppm, tmp_path):
    L, libc = ppm
    rng = np.random.default_rng(6)
    W, H, n = 37, 21, 3
    fr = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]
    fr[1][0, 0] = (ord("#"), ord("\n"), ord("P"))         # pixel bytes that look like header bytes
    path = str(tmp_path / "w.ppm")
    fp = libc.fopen(path.encode(), b"wb")
    for f in fr:
        assert L.ppm_write_frame(fp, W, H, f.ctypes.data) == OK
    libc.fclose(fp)
    raw = open(path, "rb").read()
    assert raw == _stream(fr), "the container ffmpeg -f image2pipe -vcodec ppm writes"
    got, rc = _read_all(ppm, path)
    assert rc == EOF and len(got) == n
    for a, b in zip(got, fr):
        assert np.array_equal(a, b)


def test_truncated_and_resized_frames(ppm, tmp_path):
    rng = np.random.default_rng(7)
    a, b = (rng.integers(0, 256, (5, 4, 3)).astype(np.uint8) for _ in range(2))
    other = rng.integers(0, 256, (4, 5, 3)).astype(np.uint8)   # as many bytes, another shape
    path = str(tmp_path / "s.ppm")
    for data, frames_ok, want in ((_stream([a, b])[:-1], 1, TRUNCATED),     # the last byte is missing
                                  (_stream([a])[:-30], 0, TRUNCATED),       # ... of the first frame
                                  (_stream([a, b]) + b"P6\n4 5\n", 2, HEADER),
                                  (_stream([a, other, b]), 1, SIZE),
                                  (_stream([a]) + b"P5\n4 5\n255\n" + bytes(20), 1, MAGIC),
                                  (_stream([a]) + b"P6\n4 5\n1023\n" + bytes(120), 1, MAXVAL),
                                  (_stream([a]) + b"\n", 1, MAGIC)):        # no separator between images
        with open(path, "wb") as f:
            f.write(data)
        got, rc = _read_all(ppm, path)
        assert (len(got), rc) == (frames_ok, want), (len(data), len(got), rc)


def test_null_arguments_and_swap(ppm, tmp_path):
    L, libc = ppm
    pi, buf = Info(2, 1), np.zeros(6, np.uint8)
    assert L.ppm_read_header(None, ctypes.byref(pi)) == ARG
    assert L.ppm_read_pixels(None, ctypes.byref(pi), buf.ctypes.data) == ARG
    assert L.ppm_read_next(None, ctypes.byref(pi), buf.ctypes.data) == ARG
    assert L.ppm_write_frame(None, 2, 1, buf.ctypes.data) == ARG
    path = str(tmp_path / "n.ppm")
    fp = libc.fopen(path.encode(), b"wb")
    assert L.ppm_read_header(fp, None) == ARG
    assert L.ppm_write_frame(fp, 2, 1, None) == ARG
    assert L.ppm_write_frame(fp, 0, 1, buf.ctypes.data) == ARG
    libc.fclose(fp)
    px = np.arange(12, dtype=np.uint8)
    L.ppm_swap_rb(px.ctypes.data, 4)
    assert np.array_equal(px, [2, 1, 0, 5, 4, 3, 8, 7, 6, 11, 10, 9])
    L.ppm_swap_rb(px.ctypes.data, 0)
    L.ppm_swap_rb(None, 4)
