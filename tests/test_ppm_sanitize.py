"""The binary PPM module (host/ppm.c) under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/sanitize/san_ppm.c, a stand-alone program,
built with any finding fatal (-fno-sanitize-recover=all; LeakSanitizer on).
Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "host")


def test_ppm_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_ppm")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", HOST,
                    "-o", exe, os.path.join(ROOT, "tests", "sanitize", "san_ppm.c"),
                    os.path.join(HOST, "ppm.c")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "san_ppm: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
