"""GaussianProcess<T>::RemoveSample() + Update() (include/gpr/GaussianProcess.h): removals queued for
the device and applied to its factor, driven through the test executable
(tests/cpp/gp_remove_test.cpp, built by `make cpptests`) as tests/test_gpu_append_host.py drives
gp_append_test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpr_amd", "lib")


@pytest.mark.gpu
def test_update_applies_queued_removals():
    path = os.path.join(LIB, "gp_remove_test")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, out
    assert len(lines) == 5 and all(l.startswith("PASS") for l in lines), out
