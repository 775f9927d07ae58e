"""sydr_amd/csrc/ring_format.h -- how a sample of each ring format lies in memory, read, written and dispatched -- compiled for
the host alone and checked against integer arithmetic written out in the check itself (tests/csrc/ring_format_check.hip)."""
import subprocess

import host_check


@host_check.requires_hipcc
def test_ring_formats_read_write_and_dispatch_on_the_host():
    exe = host_check.build("ring_format_check")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 65536 + 4 * 1601      # (every ci8 byte pair read, every quarter written)
