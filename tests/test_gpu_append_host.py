"""GaussianProcess<T>::Update() (include/gpr/GaussianProcess.h): the C++ host layer's opt-in
incremental Initialize(), driven through its test executable (tests/cpp/gp_append_test.cpp,
built by `make cpptests`) as tests/test_host_api.py drives gp_host_test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpr_amd", "lib")


@pytest.mark.gpu
def test_update_extends_the_device_factor():
    path = os.path.join(LIB, "gp_append_test")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, out
    assert len(lines) == 6 and all(l.startswith("PASS") for l in lines), out
