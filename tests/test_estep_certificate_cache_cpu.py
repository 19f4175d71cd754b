"""The two-part form of the E-step certificate constants (mimo_host_estep_certificate_ref once per reference pass,
mimo_host_estep_certificate_cur per certified pass; DESIGN section 4, "E-step certificates") against the public one-part function:
tests/estep_certificate_cache_check.cpp runs both on the same inputs, K in {1, 3, 4, 5, 49, 64} x D in {1, 14, 16, 32}, and
compares `out`, `table` and the return code byte for byte, under AddressSanitizer + UBSan.  A stand-alone host program: nothing
is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_estep_certificate_cache_under_asan_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "estep_certificate_cache_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-mavx2", "-mfma", "-pthread", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # is the sanitizer runtime there?  An empty program decides that, so no error of the real build can hide as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([hipcc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    build = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tests", "estep_certificate_cache_check.cpp"),
                                              os.path.join(ROOT, "mimo_amd", "csrc", "mimo_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "estep certificate cache ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
