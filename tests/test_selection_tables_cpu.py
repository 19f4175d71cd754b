"""The selection tables of mimo_selection.h on the CPU: tests/selection_tables_check.cpp builds the small tables of
mimo_estep_batched_rows and of the SVI loop and compares them word for word with tables written out by hand, and drives the index
check in front of them, under AddressSanitizer + UBSan.  A stand-alone host program: nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selection_tables_under_asan_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "selection_tables_check")
    # plain host C++ (no --offload-arch), as tests/test_theta_image_cpu.py builds its program
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "selection_tables_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "selection tables ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
