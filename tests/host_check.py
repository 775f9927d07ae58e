"""The one compile line of the host checks: a program under tests/csrc/ is a HOST build of a header the library's kernels and
its host side share (`hipcc --cuda-host-only`, no GPU), compiled with the library's contraction flag, once per process."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

requires_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@functools.lru_cache(maxsize=None)
def _bin_dir():
    path = tempfile.mkdtemp(prefix="sydr_host_check_")
    atexit.register(shutil.rmtree, path, ignore_errors=True)
    return path


@functools.lru_cache(maxsize=None)
def build(name, flags=("-O1",)):
    """The path of tests/csrc/<name>.hip compiled for the host. `flags` (a tuple) come last, so a caller's -ffp-contract wins."""
    exe = os.path.join(_bin_dir(), f"{name}.{len(os.listdir(_bin_dir()))}")
    out = subprocess.run([HIPCC, "-std=c++17", "--cuda-host-only", "-ffp-contract=off", *flags, "-o", exe,
                          os.path.join(CSRC, name + ".hip")], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError(f"hipcc failed on tests/csrc/{name}.hip (exit {out.returncode}):\n{out.stderr}")
    return exe
