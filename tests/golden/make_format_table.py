#!/usr/bin/env python3
"""Writes tests/golden/format_table.json: what the library's host-side format
code answers for every format code, recorded from a build of the commit BEFORE
a change to that code (tests/test_format_table_host.py then holds the changed
build to it).  Never run it against the code under test.

    python tests/golden/make_format_table.py <path to the earlier build's libmm355.so>

A pull request that adds a format regenerates the fixture from the build that
adds it, and says so.  No GPU is touched: the entry points recorded are pure
host arithmetic.
"""
import ctypes
import json
import os
import sys

INVALID = -1
SIZES = [(2, 2), (64, 48), (63, 47), (98, 62), (1920, 1080)]
SWEEP_SIZES = [(64, 48), (63, 47)]
INT_MAX, INT_MIN = 2**31 - 1, -2**31
SWEEP = list(range(-8, 4096)) + [1 << 12, 1 << 20, INT_MAX, INT_MIN]
# three codes that are no format, for the convert pairs
NOT_FORMATS = [-1, 12, 16 | 32 | 64]


class Surface(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int), ("pitch", ctypes.c_size_t), ("chroma_offset", ctypes.c_size_t),
                ("chroma_pitch", ctypes.c_size_t), ("frame_stride", ctypes.c_size_t)]


def _sigs(L):
    ci, sz = ctypes.c_int, ctypes.c_size_t
    ps = ctypes.POINTER(Surface)
    for name, args in {"mm_frame_bytes": [ci, ci, ci, ctypes.POINTER(sz)],
                       "mm_surface_tight": [ci, ci, ci, ps],
                       "mm_surface_aligned": [ci, ci, ci, sz, ci, ps],
                       "mm_surface_bytes": [ci, ci, ps, ctypes.POINTER(sz)],
                       "mm_ycbcr_matrix": [ci, ctypes.POINTER(ctypes.c_double * 6)],
                       "mm_convert_supported": [ci, ci]}.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ci, args


def frame_bytes(L, W, H, fmt):
    n = ctypes.c_size_t(0)
    rc = L.mm_frame_bytes(W, H, fmt, ctypes.byref(n))
    return [rc, n.value if rc == 0 else None]


def _layout(L, W, H, rc, s):
    """[rc, the four fields, [mm_surface_bytes' rc, extent]] of a layout a helper returned"""
    if rc:
        return [rc, None, None]
    n = ctypes.c_size_t(0)
    rb = L.mm_surface_bytes(W, H, ctypes.byref(s), ctypes.byref(n))
    return [rc, [s.pitch, s.chroma_offset, s.chroma_pitch, s.frame_stride], [rb, n.value if rb == 0 else None]]


def tight(L, W, H, fmt):
    s = Surface()
    return _layout(L, W, H, L.mm_surface_tight(W, H, fmt, ctypes.byref(s)), s)


def aligned(L, W, H, fmt, pitch_align, rows_align):
    s = Surface()
    return _layout(L, W, H, L.mm_surface_aligned(W, H, fmt, pitch_align, rows_align, ctypes.byref(s)), s)


def valid_codes(L):
    return [c for c in SWEEP if L.mm_frame_bytes(64, 48, c, ctypes.byref(ctypes.c_size_t(0))) != INVALID]


def unit_of(L, fmt):
    """The format's unit: the smallest pitch alignment mm_surface_aligned takes"""
    return next(a for a in range(1, 17) if aligned(L, 64, 48, fmt, a, 2)[0] != INVALID)


def aligns(unit):
    return [(256, 16), (unit, 1), (unit, 2), (unit + 1, 2), (6, 2)]


def record(L, codes=None):
    """Everything the fixture holds, asked of library L (codes: the valid codes; None: found by the sweep)"""
    _sigs(L)
    codes = valid_codes(L) if codes is None else codes
    out = {"valid_codes": codes, "formats": {}, "convert": {}}
    for c in codes:
        u = unit_of(L, c)
        m = (ctypes.c_double * 6)()
        rc = L.mm_ycbcr_matrix(c, ctypes.byref(m))
        e = {"unit": u, "matrix": [rc, [float(v).hex() for v in m] if rc == 0 else None], "sizes": {}}
        for W, H in SIZES:
            e["sizes"][f"{W}x{H}"] = {"frame_bytes": frame_bytes(L, W, H, c), "tight": tight(L, W, H, c),
                                      "aligned": [aligned(L, W, H, c, pa, ra) for pa, ra in aligns(u)]}
        out["formats"][str(c)] = e
    sides = codes + NOT_FORMATS
    out["convert_sides"] = sides
    for a in sides:   # one row per input code: the return codes over the output codes, in order
        out["convert"][str(a)] = [L.mm_convert_supported(a, b) for b in sides]
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    lib = os.path.abspath(sys.argv[1])
    rec = record(ctypes.CDLL(lib))
    rec = {"_header": "Recorded by tests/golden/make_format_table.py from a build of the PARENT of the commit that "
                      "introduced the format table (csrc/mm_format.hpp), not from the code under test.  Return codes "
                      "as the C-ABI's; matrices as hex floats.", **rec}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "format_table.json")
    with open(dst, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{dst}: {len(rec['valid_codes'])} valid codes, {os.path.getsize(dst)} bytes")
