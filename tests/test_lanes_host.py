"""Several live streams in one call (include/mm.h "Several live streams in one
call"), on the host: the six entry points are declared, built and bound, the
ABI version stays 10, and a call without a handle is refused before anything
else is looked at.  None of it touches a GPU; what a lane computes is in
test_lanes.py."""
import ctypes
import os
import re
import subprocess

import mm355
from mm355 import Surface

INVALID = -1
SYMBOLS = ("mm_set_lanes", "mm_get_lanes", "mm_process_lanes", "mm_reset_lane", "mm_get_lane_state",
           "mm_set_lane_state")


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", mm355.LIB_PATH], capture_output=True, check=True,
                         timeout=60).stdout.decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(SYMBOLS) <= exported, set(SYMBOLS) - exported


def test_symbols_are_declared_and_bound():
    assert set(SYMBOLS) <= set(mm355.abi_symbols())
    assert tuple(mm355.binding.LANES_SYMBOLS) == SYMBOLS
    assert mm355.has_lanes()
    for name in SYMBOLS:
        assert hasattr(mm355.lib(), name), name
    for name in ("set_lanes", "lanes", "process_lanes", "reset_lane", "get_lane_state", "set_lane_state"):
        assert callable(getattr(mm355.Handle, name)), name


def test_abi_version_stays_10():
    assert mm355.lib().mm_abi_version() == 10 == mm355.binding.ABI_VERSION
    assert re.search(r"^#define\s+MM_ABI_VERSION\s+10\b", open(mm355.binding.HEADER).read(), re.M)


def test_header_defines_the_lane_cap():
    txt = open(mm355.binding.HEADER).read()
    assert re.search(r"^#define\s+MM_LANES_MAX\s+64\s*$", txt, re.M)
    assert mm355.LANES_MAX == 64
    assert "Several live streams in one call" in txt


def test_null_handle_is_invalid():
    lib = mm355.lib()
    li = Surface.tight(64, 48, mm355.RGBA8)
    buf = ctypes.create_string_buffer(64 * 48 * 4)
    n = ctypes.c_int(7)
    assert lib.mm_set_lanes(None, 2) == INVALID
    assert lib.mm_get_lanes(None, ctypes.byref(n)) == INVALID and n.value == 7
    assert lib.mm_process_lanes(None, buf, ctypes.byref(li), buf, ctypes.byref(li), None) == INVALID
    assert lib.mm_reset_lane(None, -1) == INVALID
    assert lib.mm_get_lane_state(None, 0, buf, len(buf), None) == INVALID
    assert lib.mm_set_lane_state(None, 0, buf, len(buf), None) == INVALID


def test_cli_refuses_lanes_with_what_lanes_cannot_run():
    """Usage errors come before the device is touched (status 2)."""
    cli = os.path.join(os.path.dirname(os.path.dirname(mm355.LIB_PATH)), "bin", "mm_cli")
    base = ["-w", "64", "-h", "48", "-n", "6"]
    for args in (["--lanes", "0"], ["--lanes", "65"], ["--lanes", "3", "--orientations", "4"],
                 ["--lanes", "3", "--show-phase"], ["--lanes", "3", "--ring-local", "2"],
                 ["--lanes", "4"]):                       # 6 frames are no multiple of 4
        r = subprocess.run([cli] + base + args, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--lanes" in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([cli] + base + ["--lanes", "4"], capture_output=True, timeout=60)
    assert b"4" in r.stderr and b"6" in r.stderr
