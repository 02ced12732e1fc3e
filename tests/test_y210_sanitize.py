"""The Y4M module's 10-bit 4:2:2 entry points (host/y4m.c: y4m_read_header_ext,
C422p10 headers and frames, y4m_422p10_to_y210 / y4m_y210_to_422p10) under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/sanitize/san_422p10.c, a
stand-alone program, built with any finding fatal (-fno-sanitize-recover=all;
LeakSanitizer on).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "host")


def test_y4m_422p10_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_422p10")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", HOST,
                    "-o", exe, os.path.join(ROOT, "tests", "sanitize", "san_422p10.c"),
                    os.path.join(HOST, "y4m.c")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "san_422p10: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
