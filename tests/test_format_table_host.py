"""The library's host-side format code, held to what the build before the
format table (csrc/mm_format.hpp) answered: tests/golden/format_table.json,
recorded from that earlier build by tests/golden/make_format_table.py.  Sizes,
layouts, matrices (bitwise) and convert pairs of every valid code, and
MM_ERR_INVALID for every other code from -8 to 4095 and a few beyond: the sweep
is what lets a table lookup stand in for the predicates' "any other bit leaves
a base that is no format".  None of it touches a GPU."""
import ctypes
import json
import os
import sys

import pytest

import mm355

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_format_table as T   # noqa: E402  (the recorder: the test asks what the fixture asked)

with open(os.path.join(GOLDEN, "format_table.json")) as _f:
    FIX = json.load(_f)
VALID = FIX["valid_codes"]


@pytest.fixture(scope="module")
def lib():
    # a handle of its own on the same file: the recorder's signatures stay off the package's
    L = ctypes.CDLL(mm355.load_library()._name)
    T._sigs(L)
    return L


def test_the_fixture_covers_every_public_code():
    public = [mm355.RGBA8, mm355.RGBA32F, mm355.RGBA16F, mm355.RGBA8_SRGB, mm355.RGB24, mm355.BGR24,
              mm355.Y8, mm355.Y10, mm355.Y12, mm355.Y16, mm355.NV12, mm355.NV12_FULL, mm355.P010,
              mm355.P010_FULL, mm355.I420, mm355.I420_FULL, mm355.I010, mm355.I010_FULL, mm355.YUY2,
              mm355.YUY2_FULL, mm355.UYVY, mm355.UYVY_FULL, mm355.Y210, mm355.Y210_FULL]
    assert set(public) <= set(VALID)
    # 4 RGBA, 2 packed RGB, 4 single-plane, 7 Y'CbCr families x 2 ranges x (BT.601, BT.709, BT.2020)
    assert len(VALID) == 4 + 2 + 4 + 7 * 2 * 3 and len(set(VALID)) == len(VALID)


def test_every_other_code_is_invalid(lib):
    valid, bad = set(VALID), []
    n, s = ctypes.c_size_t(0), T.Surface()
    for c in T.SWEEP:
        if c in valid:
            continue
        for W, H in T.SWEEP_SIZES:
            if lib.mm_frame_bytes(W, H, c, ctypes.byref(n)) != T.INVALID:
                bad.append(("mm_frame_bytes", c, W, H))
            if lib.mm_surface_tight(W, H, c, ctypes.byref(s)) != T.INVALID:
                bad.append(("mm_surface_tight", c, W, H))
    assert not bad, bad[:20]
    assert len(T.SWEEP) == 4104 + 4


def test_the_valid_codes_are_valid(lib):
    assert T.valid_codes(lib) == VALID


@pytest.mark.parametrize("code", VALID)
def test_sizes_layouts_and_matrix_are_the_recorded_ones(lib, code):
    got = T.record(lib, codes=[code])["formats"][str(code)]
    want = FIX["formats"][str(code)]
    assert got["unit"] == want["unit"]
    assert got["matrix"] == want["matrix"]   # hex floats: bitwise
    for size in want["sizes"]:
        assert got["sizes"][size] == want["sizes"][size], size
    assert set(got["sizes"]) == set(want["sizes"]) == {f"{W}x{H}" for W, H in T.SIZES}


def test_convert_pairs_are_the_recorded_ones(lib):
    sides = FIX["convert_sides"]
    assert sides == VALID + T.NOT_FORMATS
    for a in sides:
        got = [lib.mm_convert_supported(a, b) for b in sides]
        assert got == FIX["convert"][str(a)], a
