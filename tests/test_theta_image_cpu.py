"""The Theta operand images of mimo_theta.h on the CPU: tests/theta_image_check.cpp packs every placement and reads it back
through readers written from the kernels' layout comments, under AddressSanitizer + UBSan (a write outside an image's
count() doubles is a sanitizer error).  A stand-alone host program: nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_theta_images_under_asan_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "theta_image_check")
    # plain host C++ (no --offload-arch), as mimo_host.o is built
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "theta_image_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "theta images ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
