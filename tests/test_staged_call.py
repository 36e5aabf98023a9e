"""The protocol of the blocking host-pointer entry points (csrc/bu_context.hpp, csrc/bu_staged_call.hpp) on the CPU: tests/host_emul/bu_staged_call_check.cpp
compiles the shipped text against the real HIP runtime API header and a recording runtime of its own, under ASan / UBSan.  A device-to-host copy lands at the
next synchronise of its stream, so a copy that outlives its landing area is a write into freed memory.  A model driver that uses every step is run with
pageable and page-locked buffers (the recorded call order against a literal one), with every runtime call failing in turn (BU_ERR_HIP that names the call,
nothing left in flight, the lock free, the next call on the context right), with status words of several images, and with page-locked buffers whose device
view is not aligned as the step asks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")


def test_staged_call_under_sanitizers():
    subprocess.run(["make", "-C", HOST_EMUL, "bu_staged_call_asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(HOST_EMUL, "bu_staged_call_asan")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr[-3000:]
    for part in ("order ok", "failures ok", "status ok", "alignment ok", "staged call check done"):
        assert part in r.stdout, r.stdout
