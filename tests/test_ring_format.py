"""sydr_amd/csrc/ring_format.h -- how a sample of each ring format lies in memory, read, written and dispatched -- compiled for
the host alone and checked against integer arithmetic written out in the check itself (tests/csrc/ring_format_check.hip)."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ring_formats_read_write_and_dispatch_on_the_host(tmp_path):
    exe = tmp_path / "ring_format_check"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--cuda-host-only", "-o", str(exe),
                           os.path.join(REPO, "tests", "csrc", "ring_format_check.hip")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 65536 + 4 * 1601      # (every ci8 byte pair read, every quarter written)
