"""The timers build (libvio_hip_timers.so, `make -C vins-rgbd-fast_amd/csrc timers`: the same sources with the in-kernel phase timers compiled in) against
the shipped library on three short runs: same priors, reboots and iteration counts.  Different register allocation and timing -- a difference between the two
is a race or an undefined behaviour in the kernels (round 6: it exposed a rewritten block_scan_flags that every other test had passed).  The test builds
the timers library itself (it is a profiling tool, __graft_entry__.build() does not make it)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timers_build_computes_what_the_shipped_library_computes():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "vins-rgbd-fast_amd", "csrc"), "timers"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "timers_sanity.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-500:]
