"""CPU: the device / host split of PROSAC's termination scan for multi-problem batches.  The kernel's
half restated on the host (flags -> counts -> non_random update -> ordered candidates) plus
usac::ProsacTerminationCriteria::applyCandidates give the plain scan's bound and termination length
on every call (tests/cpp_multi_prosac/scan_split_check.cpp, g++ against the host header only -- no
GPU, no HIP)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_scan_split_equals_plain(tmp_path):
    exe = str(tmp_path / "scan_split_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ransac_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp_multi_prosac", "scan_split_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
