"""A subset of the lanes per call (include/mm.h "Several live streams in one
call": mm_process_lanes_mask, mm_lanes_with_state), on the host: the two entry
points are declared, built and bound in a tuple of their own, a call without a
handle is refused before anything else is looked at, and mm_cli refuses a
--lane-drop it cannot run before it creates the output file.  None of it
touches a GPU; what a mask call computes is in test_lanes_mask.py."""
import ctypes
import os
import re
import subprocess

import pytest

import mm355
from mm355 import Surface

INVALID = -1
SYMBOLS = ("mm_process_lanes_mask", "mm_lanes_with_state")


def test_symbols_are_declared_and_exported():
    assert set(SYMBOLS) <= set(mm355.abi_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", mm355.LIB_PATH], capture_output=True, check=True,
                         timeout=60).stdout.decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(SYMBOLS) <= exported, set(SYMBOLS) - exported


def test_symbols_are_bound_in_a_tuple_of_their_own():
    assert tuple(mm355.binding.LANES_MASK_SYMBOLS) == SYMBOLS
    assert not set(SYMBOLS) & set(mm355.binding.LANES_SYMBOLS)      # an older library still answers has_lanes()
    assert mm355.has_lanes_mask() and mm355.has_lanes()
    for name in SYMBOLS:
        assert hasattr(mm355.lib(), name), name
    for name in ("process_lanes_mask", "lanes_with_state"):
        assert callable(getattr(mm355.Handle, name)), name


def test_header_documents_the_mask_calls():
    txt = open(mm355.binding.HEADER).read()
    assert re.search(r"^#define\s+MM_ABI_VERSION\s+10\b", txt, re.M) and mm355.lib().mm_abi_version() == 10
    assert re.search(r"int\s+mm_process_lanes_mask\(mm_handle \*h, uint64_t mask,", txt)
    assert re.search(r"int\s+mm_lanes_with_state\(const mm_handle \*h, uint64_t \*mask\);", txt)
    assert "calls that advance a subset of the lanes" not in txt          # no longer out of scope


def test_null_handle_is_invalid():
    lib = mm355.lib()
    li = Surface.tight(64, 48, mm355.RGBA8)
    buf = ctypes.create_string_buffer(64 * 48 * 4)
    m = ctypes.c_uint64(7)
    assert lib.mm_process_lanes_mask(None, 1, buf, ctypes.byref(li), buf, ctypes.byref(li), None) == INVALID
    assert lib.mm_process_lanes_mask(None, 0, None, ctypes.byref(li), None, ctypes.byref(li), None) == INVALID
    assert lib.mm_lanes_with_state(None, ctypes.byref(m)) == INVALID and m.value == 7


@pytest.mark.parametrize("args,word", [
    (["--lane-drop", "1:2"], b"needs --lanes"),                            # without --lanes
    (["--lanes", "2", "--lane-drop", "2:0"], b"takes L:T"),          # a lane >= M
    (["--lanes", "2", "--lane-drop", "0:1,2:1"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", "1"], b"takes L:T"),            # malformed lists
    (["--lanes", "2", "--lane-drop", "1:"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", ":1"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", "1:2,"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", "1:2;0:1"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", "-1:2"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", "1:x"], b"takes L:T"),
    (["--lanes", "2", "--lane-drop", "0x1:2"], b"takes L:T"),
], ids=lambda v: "_".join(v) if isinstance(v, list) else None)
def test_cli_refuses_a_lane_drop_it_cannot_run(tmp_path, args, word):
    """Usage errors: status 2 before the device is touched, and no output file.
    The words are the --lane-drop parser's own (a driver without the option says
    "unknown option" with the same status)."""
    cli = os.path.join(os.path.dirname(os.path.dirname(mm355.LIB_PATH)), "bin", "mm_cli")
    src, dst = str(tmp_path / "in.rgba"), str(tmp_path / "out.rgba")
    with open(src, "wb") as f:
        f.write(bytes(64 * 48 * 4 * 4))
    r = subprocess.run([cli, "-w", "64", "-h", "48", "-i", src, "-o", dst] + args, capture_output=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    assert not os.path.exists(dst)
