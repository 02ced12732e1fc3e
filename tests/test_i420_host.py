"""MM_I420 / MM_I420_FULL on the host (no GPU): the plane-layout bit and the six
codes, sizes and surface rules in the C ABI (the derived Cr plane included), the
Python layer's shapes, the test-side helpers (tests/i420.py) and the
command-line driver's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import i420
import mm355

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phase-based-motion-manipulation_amd")
CLI = os.path.join(PKG, "bin", "mm_cli")
OK, INVALID, UNSUPPORTED = 0, -1, -2
CODES = (528, 529, 560, 561, 592, 593)
# the bit by itself (RGBA8 | 512), on every other family, with the order bit,
# both matrix bits, any other stray bit
BAD_CODES = (512, 1 | 512, 2 | 512, 3 | 512, 8 | 512, 11 | 512, 18 | 512, 19 | 512, 24 | 512, 26 | 512, 22 | 512,
             13 | 512, 141 | 512, 528 | 128, 528 | 32 | 64, 529 | 96, 528 | 256, 528 | 1024, -528)


def _code(call):
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def test_format_codes_and_frame_bytes():
    assert (mm355.PLANAR, mm355.I420, mm355.I420_FULL) == (512, 528, 529)
    assert mm355.I420_FORMATS == (528, 529)
    for name in ("I420", "I420_FULL", "PLANAR", "I420_FORMATS"):
        assert name in mm355.__all__
    hdr = open(mm355.binding.HEADER).read()
    assert any(ln.split()[:3] == ["#define", "MM_PLANAR", "512"] for ln in hdr.splitlines())
    assert any(ln.split()[:5] == ["#define", "MM_I420", "(MM_NV12", "|", "MM_PLANAR)"] for ln in hdr.splitlines())
    assert any(ln.split()[:5] == ["#define", "MM_I420_FULL", "(MM_NV12_FULL", "|", "MM_PLANAR)"]
               for ln in hdr.splitlines())
    assert mm355.lib().mm_abi_version() == 10            # a backward-compatible addition
    for c in CODES:
        assert mm355.frame_bytes(1920, 1080, c) == 3110400, c
        assert mm355.frame_bytes(98, 62, c) == 9114, c
        assert mm355.base_format(c) in mm355.I420_FORMATS    # the planar bit stays, the matrix bit goes
    assert mm355.I420 not in mm355.FORMAT_BPP             # as the other 4:2:0 codes


def test_every_invalid_code_is_refused_everywhere():
    n = ctypes.c_size_t()
    for bad in BAD_CODES:
        assert _code(lambda: mm355.frame_bytes(64, 48, bad)) == INVALID, bad
        assert _code(lambda: mm355.Surface.tight(64, 48, bad)) == INVALID, bad
        assert _code(lambda: mm355.Surface.aligned(64, 48, bad)) == INVALID, bad
        s = mm355.Surface.tight(64, 48, mm355.I420)
        s.format = bad
        assert mm355.lib().mm_surface_bytes(64, 48, ctypes.byref(s), ctypes.byref(n)) == INVALID, bad
        assert mm355.lib().mm_process(None, None, None, bad, 0, None) == INVALID, bad
        assert mm355.convert_supported(bad, bad) == INVALID, bad


def test_odd_sizes_are_unsupported():
    for c in CODES:
        for W, H in ((97, 62), (98, 63), (97, 63)):
            assert _code(lambda: mm355.frame_bytes(W, H, c)) == UNSUPPORTED
            assert _code(lambda: mm355.Surface.tight(W, H, c)) == UNSUPPORTED
            assert _code(lambda: mm355.Surface.aligned(W, H, c)) == UNSUPPORTED


def test_surface_figures():
    for c in CODES:
        t = mm355.Surface.tight(1920, 1080, c)
        assert (t.format, t.pitch, t.chroma_offset, t.chroma_pitch, t.frame_stride) == (c, 1920, 2073600, 960, 3110400)
        assert t.bytes(1920, 1080) == 3110400
        t = mm355.Surface.tight(98, 62, c)
        assert (t.pitch, t.chroma_offset, t.chroma_pitch, t.frame_stride) == (98, 6076, 49, 9114)
        assert t.chroma_offset + t.chroma_pitch * 31 == 7595          # the Cr plane
        assert t.bytes(98, 62) == 9114 == i420.extent(98, 62, t)
        a = mm355.Surface.aligned(1920, 1080, c, 256, 16)
        assert (a.format, a.pitch, a.chroma_offset, a.chroma_pitch, a.frame_stride) == (c, 2048, 2228224, 1024, 3342336)
        assert a.chroma_offset + a.chroma_pitch * 540 == 2781184      # the Cr plane
        assert a.bytes(1920, 1080) == 3334080 == i420.extent(1920, 1080, a)
    # an odd rounded pitch has no half; odd rows_align splits no chroma row pairs
    assert _code(lambda: mm355.Surface.aligned(98, 62, mm355.I420, 33, 2)) == INVALID      # pitch 99
    assert mm355.Surface.aligned(98, 62, mm355.I420, 34, 2).chroma_pitch == 51             # pitch 102
    assert _code(lambda: mm355.Surface.aligned(98, 62, mm355.I420, 2, 3)) == INVALID


def test_surface_rules_one_byte_short_of_legal():
    W, H = 98, 62
    for c in (mm355.I420, mm355.I420_FULL | mm355.MATRIX_BT709):
        t = mm355.Surface.tight(W, H, c)
        ok = i420.layout(c, W + 1, W * H + (H - 1) + 3, W // 2 + 1)    # unit 1: odd pitches, an offset anywhere past the luma
        assert ok.bytes(W, H) == i420.extent(W, H, ok)
        assert _code(lambda: i420.layout(c, W - 1, t.chroma_offset, t.chroma_pitch).bytes(W, H)) == INVALID
        assert _code(lambda: i420.layout(c, W, t.chroma_offset, W // 2 - 1).bytes(W, H)) == INVALID
        assert _code(lambda: i420.layout(c, W, t.chroma_offset - 1, t.chroma_pitch).bytes(W, H)) == INVALID   # inside the luma plane
        assert _code(lambda: i420.layout(c, W, 0, t.chroma_pitch).bytes(W, H)) == INVALID
        # size_t overflow and the 4 GiB rule
        assert _code(lambda: i420.layout(c, W, t.chroma_offset, 2 ** 63).bytes(W, H)) == INVALID
        assert _code(lambda: i420.layout(c, W, 2 ** 64 - 100, t.chroma_pitch).bytes(W, H)) == INVALID
        assert _code(lambda: i420.layout(c, W, 2 ** 32, t.chroma_pitch).bytes(W, H)) == UNSUPPORTED
    # frame_stride = extent - 1 with two frames: mm_process_stream_surfaces refuses it before
    # touching the handle's device (no handle here: the stride rule is checked on a live
    # handle in test_i420.py); the extent the rule compares with is the one above
    t = mm355.Surface.tight(W, H, mm355.I420)
    assert t.frame_stride == t.bytes(W, H)


def test_matrix_and_convert_tables():
    for c in CODES:
        assert np.array_equal(mm355.ycbcr_matrix(c), mm355.ycbcr_matrix(i420.nv12_code(c))), c
        assert mm355.convert_supported(c, c) == OK
        for other in (0, 16, 17, 18, 48, 1, 13, 24, c ^ 1):
            assert mm355.convert_supported(c, other) == UNSUPPORTED, (c, other)
            assert mm355.convert_supported(other, c) == UNSUPPORTED, (other, c)
    assert mm355.convert_supported(528, 528) == 0
    assert mm355.convert_supported(528, 0) == mm355.convert_supported(0, 528) == mm355.convert_supported(528, 16) == -2
    assert _code(lambda: mm355.ycbcr_matrix(512)) == INVALID


class _Recorder:
    """Stands in for the handle: records what OnRenderImage would call."""

    def __init__(self):
        self.calls = []

    def process(self, *a, **kw):
        self.calls.append(("process", a, kw))

    def process_surface(self, *a, **kw):
        self.calls.append(("process_surface", a, kw))


def test_on_render_image_shapes_and_dtypes():
    W, H = 64, 48
    a = mm355.processor.host_frames(3, H, W, mm355.I420 | mm355.MATRIX_BT2020)
    assert a.shape == (3, H * 3 // 2, W) and a.dtype == np.uint8
    proc = mm355.MotionMagnificationProcessor(W, H)
    proc._handle = rec = _Recorder()
    fr = np.zeros((H * 3 // 2, W), np.uint8)
    try:
        for c in CODES:
            proc.OnRenderImage(fr, fr.copy(), fmt=c)
            name, args, kw = rec.calls[-1]
            assert name == "process" and args[0] is fr and args[2] == c and kw["on_device"] is False
        n = len(rec.calls)
        bad = [np.zeros((H * 3 // 2, W), np.uint16),            # words
               np.zeros((H, W), np.uint8),                      # the luma plane alone
               np.zeros((H * 3 // 2, W, 1), np.uint8),
               np.zeros((H, W, 4), np.uint8),                   # an RGBA8 frame
               np.zeros(H * 3 // 2 * W, np.uint8),              # flat
               np.zeros((H * 3, W), np.uint8)[::2],             # row-strided
               np.zeros((H * 3 // 2, 2 * W), np.uint8)[:, ::2],
               np.zeros((H * 3 // 2, W + 8), np.uint8)[:, :W]]  # a region of a wider parent
        for b in bad:
            assert _code(lambda: proc.OnRenderImage(b, fr.copy(), fmt=mm355.I420)) == INVALID
            assert _code(lambda: proc.OnRenderImage(fr, b, fmt=mm355.I420_FULL)) == INVALID
        assert len(rec.calls) == n                    # nothing reached the library
    finally:
        proc._handle = None


def test_helpers_hand_values():
    W, H = 4, 2
    nv = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [10, 20, 11, 21]], np.uint8)
    p = i420.from_nv12(nv)
    assert p.shape == nv.shape and p.reshape(-1).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 20, 21]
    assert np.array_equal(i420.to_nv12(p), nv)
    rng = np.random.default_rng(1)
    big = rng.integers(0, 256, (62 * 3 // 2, 98), dtype=np.uint8)
    assert np.array_equal(i420.to_nv12(i420.from_nv12(big)), big)
    assert np.array_equal(np.sort(i420.from_nv12(big).reshape(-1)), np.sort(big.reshape(-1)))
    lay = i420.layout(mm355.I420, 5, 11, 3, 40)
    fr = [p.reshape(-1), p.reshape(-1) + 100]
    buf = i420.scatter(W, H, fr, lay, base=1)
    assert buf[0] == i420.POISON and buf[1:5].tolist() == [1, 2, 3, 4] and buf[5] == i420.POISON
    assert buf[6:10].tolist() == [5, 6, 7, 8]
    assert buf[12:14].tolist() == [10, 11] and buf[14] == i420.POISON and buf[15:17].tolist() == [20, 21]   # Cr: 11 + 3 * 1
    assert buf[41:45].tolist() == [101, 102, 103, 104]
    m = i420.sample_mask(W, H, lay, 2, buf.size, base=1)
    assert int(m.sum()) == 2 * 12 and np.all(buf[~m] == i420.POISON)
    got = i420.gather(W, H, buf, lay, 2, base=1)
    assert np.array_equal(got[0], fr[0]) and np.array_equal(got[1], fr[1])
    assert i420.extent(W, H, lay) == 11 + 3 + 2 == lay.bytes(W, H)


def _y4m(path, tag="C420", W=16, H=16, nbytes=None):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 {tag}\n".encode() + b"FRAME\n" +
                bytes(W * H * 3 // 2 if nbytes is None else nbytes))


def test_cli_refusals(tmp_path):
    """Refused combinations end with the usage status (2) and a message that
    names --i420, before any device is touched, and write nothing: the output
    file is not even created."""
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-s", "-C", PKG])
    ok, out = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    _y4m(ok)
    c444, c422, c10, odd, mono = (str(tmp_path / n) for n in ("444.y4m", "422.y4m", "p10.y4m", "odd.y4m", "mono.y4m"))
    _y4m(c444, "C444", nbytes=16 * 16 * 3)
    _y4m(c422, "C422", nbytes=16 * 16 * 2)
    _y4m(c10, "C420p10", nbytes=16 * 16 * 3)
    _y4m(mono, "Cmono", nbytes=16 * 16)
    _y4m(odd, "C420", W=15, H=16, nbytes=15 * 16 + 2 * 8 * 8)
    raw = str(tmp_path / "in.yuv")
    with open(raw, "wb") as f:
        f.write(bytes(15 * 16 * 2))
    cases = [["--i420"],                                                   # no input at all
             ["--i420", "-i", ok, "--nv12"], ["--i420", "-i", ok, "--p010"], ["--i420", "-i", ok, "--mono"],
             ["--i420", "-i", ok, "--yuy2"], ["--i420", "-i", ok, "--uyvy"], ["--i420", "-i", ok, "--y210"],
             ["--i420", "-i", ok, "--ppm"], ["--i420", "-i", ok, "--out-rgba8"], ["--i420", "-i", ok, "--out-nv12"],
             ["--i420", "-i", ok, "--srgb"], ["--i420", "-i", ok, "--show-phase"],
             ["--i420", "-i", ok, "--show-magnitude"], ["--i420", "-i", ok, "--ring-local", "2"],
             ["--i420", "-i", ok, "--ring-world", "2"],
             ["--i420", "-i", ok, "--matrix", "470"],
             ["--i420", "-i", c444], ["--i420", "-i", c422], ["--i420", "-i", c10], ["--i420", "-i", mono],
             ["--i420", "-i", odd],                                        # odd width
             ["--i420", "-i", raw, "-w", "15", "-h", "16"]]                # ... of raw frames
    for args in cases:
        r = subprocess.run([CLI] + args + ["-o", out, "-n", "1"], capture_output=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert b"--i420" in r.stderr, (args, r.stderr)
        assert not os.path.exists(out), args
