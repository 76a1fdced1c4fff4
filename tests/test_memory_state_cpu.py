"""The LTM memory's host-side bookkeeping without a GPU (``csrc/ltm_memory_state.h``): every named transition from a fresh state
and from the state a fused call leaves, the 36 ordered pairs of the six kinds of operation, and the two orders that went wrong
before (a layer import behind an unconsumed chain import; what a forget leaves alone) -- all against expectations written out in
``tools/memory_state_host_check.cpp``, a program of its own built under the address and undefined-behaviour sanitizers."""
from __future__ import annotations

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transitions_in_a_sanitized_host_program(tmp_path):
    """The header needs no HIP: a plain C++ line builds the program; nothing is loaded into Python and nothing is preloaded."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the host check"
    exe = str(tmp_path / "memory_state_host_check")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined",
           os.path.join(ROOT, "tools", "memory_state_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr[-4000:]
    assert "memory state host check: ok" in ran.stdout
    assert "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
