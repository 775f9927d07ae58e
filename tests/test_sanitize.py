"""every program under tests/csrc/ -- the host halves that parse untrusted input or are shared with the
device -- runs clean under the address and undefined-behaviour sanitizers: `make -C sydr_amd/csrc check-sanitize` (stand-alone
programs on the CPU only).  Each program's own header comment says what it checks."""
import os
import subprocess

from host_check import requires_hipcc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@requires_hipcc
def test_host_halves_are_clean_under_asan_and_ubsan(tmp_path):
    jobs = min(16, len(os.sched_getaffinity(0)))
    out = subprocess.run(["make", "-C", os.path.join(REPO, "sydr_amd", "csrc"), f"-j{jobs}", "check-sanitize", f"SAN_DIR={tmp_path}"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "check-sanitize: clean" in out.stdout
    assert "runtime error" not in out.stdout + out.stderr and "AddressSanitizer" not in out.stdout + out.stderr
