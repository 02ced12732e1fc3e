"""The matrix bits MM_MATRIX_BT709 / MM_MATRIX_BT2020 on the host (no GPU): the
format codes the C ABI accepts and refuses, their sizes and surfaces,
mm_ycbcr_matrix against its float64 definition, and the test-side codec
(tests/ycbcr.py) pinned, for matrix 601, to tests/nv12.py and tests/p010.py."""
import ctypes

import numpy as np
import pytest

import mm355
import mmtest as T
import nv12
import p010
import ycbcr

BASES = (mm355.NV12, mm355.NV12_FULL, mm355.P010, mm355.P010_FULL)
BITS = (mm355.MATRIX_BT709, mm355.MATRIX_BT2020)
MATRIXED = [b | m for m in BITS for b in BASES]
RGBA = (mm355.RGBA8, mm355.RGBA32F, mm355.RGBA16F, mm355.RGBA8_SRGB)
INVALID = ([f | m for f in RGBA for m in BITS] +                                  # a matrix bit on an RGBA format
           [b | mm355.MATRIX_BT709 | mm355.MATRIX_BT2020 for b in BASES] +        # both bits together
           [b | 128 for b in BASES] + [b | 128 | mm355.MATRIX_BT709 for b in BASES] +   # bit 128
           [mm355.MATRIX_BT709, mm355.MATRIX_BT2020, 20 | mm355.MATRIX_BT709])    # no 4:2:0 base


def _code(call):
    with pytest.raises(mm355.MMError) as ei:
        call()
    return ei.value.code


def test_codes_and_header():
    assert (mm355.MATRIX_BT709, mm355.MATRIX_BT2020) == (32, 64)
    assert "MATRIX_BT709" in mm355.__all__ and "MATRIX_BT2020" in mm355.__all__ and "ycbcr_matrix" in mm355.__all__
    assert sorted(MATRIXED) == list(range(48, 52)) + list(range(80, 84))
    hdr = open(mm355.binding.HEADER).read()
    assert "#define MM_MATRIX_BT709   32" in hdr and "#define MM_MATRIX_BT2020  64" in hdr
    assert mm355.lib().mm_abi_version() == 10
    assert "mm_ycbcr_matrix" in mm355.abi_symbols() and hasattr(mm355.lib(), "mm_ycbcr_matrix")
    assert [ycbcr.fmt_code(m, f, d) for m in (709, 2020) for d in (8, 10) for f in (False, True)] == MATRIXED


@pytest.mark.parametrize("fmt", MATRIXED)
def test_matrixed_codes_have_their_base_formats_sizes(fmt):
    base = mm355.base_format(fmt)
    assert base in BASES
    for W, H in ((1920, 1080), (98, 62), (64, 48)):
        assert mm355.frame_bytes(W, H, fmt) == mm355.frame_bytes(W, H, base)
        t, tb = mm355.Surface.tight(W, H, fmt), mm355.Surface.tight(W, H, base)
        a, ab = mm355.Surface.aligned(W, H, fmt, 256, 16), mm355.Surface.aligned(W, H, base, 256, 16)
        for s, sb in ((t, tb), (a, ab)):
            assert s.format == fmt
            assert (s.pitch, s.chroma_offset, s.chroma_pitch, s.frame_stride) == \
                   (sb.pitch, sb.chroma_offset, sb.chroma_pitch, sb.frame_stride)
            assert s.bytes(W, H) == sb.bytes(W, H)
    assert mm355.frame_bytes(1920, 1080, fmt) == (3110400 if base < mm355.P010 else 6220800)
    # the surface units stay 2 (NV12) and 4 (P010)
    u = 2 if base < mm355.P010 else 4
    s = mm355.Surface.tight(64, 48, fmt)
    s.pitch += u
    s.chroma_offset += 48 * u
    s.chroma_pitch += u
    assert s.bytes(64, 48) > 0
    s.pitch += u // 2
    assert _code(lambda: s.bytes(64, 48)) == -1
    # odd W or H is still "unsupported", not "invalid"
    for W, H in ((97, 63), (98, 63), (97, 62)):
        assert _code(lambda: mm355.frame_bytes(W, H, fmt)) == -2
        assert _code(lambda: mm355.Surface.tight(W, H, fmt)) == -2
        assert _code(lambda: mm355.Surface.aligned(W, H, fmt, 256, 16)) == -2
    # shapes of the host-side frame arrays
    hf = mm355.processor.host_frames(2, 48, 64, fmt)
    assert hf.shape == (2, 72, 64) and hf.dtype == (np.uint8 if base < mm355.P010 else np.uint16)


@pytest.mark.parametrize("fmt", INVALID)
def test_invalid_combinations_are_refused(fmt):
    assert _code(lambda: mm355.frame_bytes(64, 48, fmt)) == -1
    assert _code(lambda: mm355.frame_bytes(97, 63, fmt)) == -1      # invalid before unsupported
    assert _code(lambda: mm355.Surface.tight(64, 48, fmt)) == -1
    assert _code(lambda: mm355.Surface.aligned(64, 48, fmt, 256, 16)) == -1
    s = mm355.Surface.tight(64, 48, mm355.NV12)
    s.format = fmt
    assert _code(lambda: s.bytes(64, 48)) == -1
    assert _code(lambda: mm355.ycbcr_matrix(fmt)) == -1
    # a frame entry point refuses the code before it looks at anything else
    assert mm355.lib().mm_process(None, None, None, fmt, 0, None) == -1


def test_ycbcr_matrix_is_the_float64_product():
    for fmt in BASES:
        m = mm355.ycbcr_matrix(fmt)
        assert m.shape == (3, 2)
        assert m[0, 0] == 0.0 and m[0, 1] == 0.0                     # exactly: BT.601's luma IS RGBToYIQ's
        assert np.array_equal(m[1:], mm355.nv12_chroma_matrix())
        assert np.array_equal(m, ycbcr.matrix_yiq(601)) or np.abs(m - ycbcr.matrix_yiq(601)).max() <= 1e-12
    for matrix in (709, 2020):
        want = ycbcr.matrix_yiq(matrix)
        kr, kb = ycbcr.KRKB[matrix]
        kg = 1.0 - kr - kb
        a = 0.114 * 2 * (1 - kb) - 0.587 * 2 * kb * (1 - kb) / kg
        b = 0.299 * 2 * (1 - kr) - 0.587 * 2 * kr * (1 - kr) / kg
        for full in (False, True):
            for depth in (8, 10):
                m = mm355.ycbcr_matrix(ycbcr.fmt_code(matrix, full, depth))
                assert np.abs(m - want).max() <= 1e-12
                assert abs(m[0, 0] - a) <= 1e-12 and abs(m[0, 1] - b) <= 1e-12
        # the I and Q rows of RGBToYIQ sum to 0: no y column, whatever the matrix
        assert abs(ycbcr.YIQ[1].sum()) < 1e-15 and abs(ycbcr.YIQ[2].sum()) < 1e-15
    m709 = mm355.ycbcr_matrix(mm355.NV12 | mm355.MATRIX_BT709)
    assert abs(m709[0, 0] - 0.10158) < 5e-6 and abs(m709[0, 1] - 0.19608) < 5e-6
    for fmt in RGBA + (4, 15, 20):
        assert _code(lambda: mm355.ycbcr_matrix(fmt)) == -1
    assert mm355.lib().mm_ycbcr_matrix(mm355.NV12 | mm355.MATRIX_BT709, None) == -1


def test_ycbcr_helper_matrix_601_is_the_nv12_and_p010_helpers():
    W, H = 70, 46
    rng = np.random.default_rng(709)
    for t, rgb in enumerate(T.synth(W, H, 2, fmt="u8")):
        for full in (False, True):
            b8, b10 = nv12.encode(rgb, full=full), p010.encode(rgb, full=full)
            assert np.array_equal(ycbcr.encode(rgb, 601, full, 8), b8)
            assert np.array_equal(ycbcr.encode(rgb, 601, full, 10), b10)
            s8, s10 = nv12.chroma_stress(b8, t), p010.chroma_stress(b10, t)
            assert np.array_equal(ycbcr.chroma_stress(b8, t, 8), s8)
            assert np.array_equal(ycbcr.chroma_stress(b10, t, 10), s10)
            s10 = s10 | rng.integers(0, 64, s10.shape).astype(np.uint16)      # P016-style low bits
            for dt in (np.float32, np.float64):
                d8, d10 = nv12.decode(s8, dt, full=full), p010.decode(s10, dt, full=full)
                assert np.array_equal(ycbcr.decode(s8, dt, 601, full, 8), d8)
                assert np.array_equal(ycbcr.decode(s10, dt, 601, full, 10), d10)
            # float frames, out of gamut: the saturate and the 2 x 2 mean
            f = nv12.decode(s8, np.float32, full=full)
            assert np.array_equal(ycbcr.encode(f, 601, full, 8), nv12.encode(f, full=full))
            assert np.array_equal(ycbcr.encode(f, 601, full, 10), p010.encode(f, full=full))


def test_ycbcr_helper_round_trips_and_matrices_differ():
    """encode(decode(frame)) is the frame for in-gamut content under every
    matrix, and the three matrices read the same bytes as different pixels."""
    W, H = 64, 48
    rgb = T.synth(W, H, 1, fmt="u8")[0]
    for depth in (8, 10):
        for full in (False, True):
            dec = {}
            for matrix in ycbcr.MATRICES:
                buf = ycbcr.encode(rgb, matrix, full, depth)
                flat = ycbcr.encode(np.repeat(np.repeat(rgb[::2, ::2], 2, 0), 2, 1), matrix, full, depth)
                back = ycbcr.encode(ycbcr.decode(flat, np.float64, matrix, full, depth), matrix, full, depth)
                assert np.array_equal(back, flat), (matrix, full, depth)
                dec[matrix] = ycbcr.decode(ycbcr.encode(rgb, 601, full, depth), np.float64, matrix, full, depth)
                # neutral chroma: R = G = B = y under every matrix
                g = buf.copy()
                g[H:] = 128 if depth == 8 else 0x8000
                d = ycbcr.decode(g, np.float64, matrix, full, depth)
                assert np.array_equal(d[..., 0], d[..., 1]) and np.array_equal(d[..., 1], d[..., 2])
            assert np.abs(dec[709] - dec[601]).max() > 0.01 and np.abs(dec[2020] - dec[709]).max() > 0.005
