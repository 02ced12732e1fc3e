"""A held reference frame (include/mm.h "Held reference frame"), on the host:
the four entry points are declared, built and bound, the ABI version stays 10,
and a call without a handle or without an out-pointer is refused before anything
else is looked at.  None of it touches a GPU; what a held stream computes is in
test_hold.py."""
import ctypes
import os
import re
import subprocess

import mm355

INVALID = -1
SYMBOLS = ("mm_set_hold", "mm_get_hold", "mm_set_lanes_hold", "mm_get_lanes_hold")


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", mm355.LIB_PATH], capture_output=True, check=True,
                         timeout=60).stdout.decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(SYMBOLS) <= exported, set(SYMBOLS) - exported


def test_symbols_are_declared_and_bound():
    assert set(SYMBOLS) <= set(mm355.abi_symbols())
    assert tuple(mm355.binding.HOLD_SYMBOLS) == SYMBOLS
    assert mm355.has_hold()
    for name in SYMBOLS:
        assert hasattr(mm355.lib(), name), name
    for name in ("set_hold", "hold", "set_lanes_hold", "lanes_hold"):
        assert callable(getattr(mm355.Handle, name)), name
    assert callable(mm355.MotionMagnificationProcessor.rehold)
    assert mm355.MotionMagnificationProcessor(64, 48).hold_reference is False
    assert mm355.MotionMagnificationProcessor(64, 48, hold_reference=True).hold_reference is True


def test_header_section_and_abi_version():
    txt = open(mm355.binding.HEADER).read()
    assert "Held reference frame" in txt
    assert mm355.lib().mm_abi_version() == 10 == mm355.binding.ABI_VERSION
    assert re.search(r"^#define\s+MM_ABI_VERSION\s+10\b", txt, re.M)


def test_null_handle_and_null_out_pointer_are_invalid():
    lib = mm355.lib()
    n = ctypes.c_int(7)
    m = ctypes.c_uint64(7)
    assert lib.mm_set_hold(None, 1) == INVALID
    assert lib.mm_get_hold(None, ctypes.byref(n)) == INVALID and n.value == 7
    assert lib.mm_set_lanes_hold(None, 1) == INVALID
    assert lib.mm_get_lanes_hold(None, ctypes.byref(m)) == INVALID and m.value == 7
    assert lib.mm_get_hold(None, None) == INVALID
    assert lib.mm_get_lanes_hold(None, None) == INVALID
    # a null out-pointer with a handle: refused before the handle is read (no
    # GPU here, so the "handle" is zeroed host memory that nothing may touch)
    fake = ctypes.create_string_buffer(1 << 16)
    assert lib.mm_get_hold(fake, None) == INVALID
    assert lib.mm_get_lanes_hold(fake, None) == INVALID
    assert fake.raw == bytes(1 << 16)


def test_cli_refuses_hold_with_what_hold_cannot_run():
    """Usage errors come before the device is touched (status 2)."""
    cli = os.path.join(os.path.dirname(os.path.dirname(mm355.LIB_PATH)), "bin", "mm_cli")
    base = ["-w", "64", "-h", "48", "-n", "6"]
    for args in (["--hold", "-1"], ["--hold", "x"], ["--hold", "3x"], ["--hold", ""]):
        r = subprocess.run([cli] + base + args, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--hold takes" in r.stderr, (args, r.returncode, r.stderr)
    for args in (["--hold", "0", "--orientations", "4"], ["--hold", "2", "--iir"],
                 ["--hold", "0", "--show-phase"], ["--hold", "0", "--show-magnitude"],
                 ["--hold", "3", "--ring-local", "2"]):
        r = subprocess.run([cli] + base + args, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--hold does not go with" in r.stderr, (args, r.returncode, r.stderr)
    # what --hold goes with is not refused where the options are read: the run gets
    # as far as the device (status 0 with a GPU, 1 without one, never a usage error)
    for args in (["--hold", "0"], ["--hold", "2", "--lanes", "3"], ["--hold", "4", "--standard"]):
        r = subprocess.run([cli] + base + args, capture_output=True, timeout=120)
        assert r.returncode in (0, 1) and b"--hold" not in r.stderr, (args, r.returncode, r.stderr)
