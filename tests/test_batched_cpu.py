"""CPU: the batched softmax pass without a GPU — the barrier / LDS-drain check of mimo_batched.hip's ISA (the check
tests/test_kernel_isa.py runs on the other kernel files), loud failures of the new entry points, and the argument
validation of BatchedHipEngine that happens before any library call."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_batched_barriers_are_reached_with_lds_drained(tmp_path, monkeypatch):
    asm = str(tmp_path / "mimo_batched.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fno-honor-nans",
           "-Wno-unused-function", "-S", "-o", asm, os.path.join(ROOT, "mimo_amd", "csrc", "mimo_batched.hip")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    import check_barrier_waits as cbw
    kernels = cbw.kernels_of(asm)
    assert len(kernels) >= 19, "kernel symbols not found in the assembly"     # 18 pass instantiations + the reduction
    bad = {k: v for k, v in ((k, cbw.check(L)) for k, L in kernels.items()) if v}
    assert not bad, f"{len(bad)} kernels reach an s_barrier with LDS operations pending, e.g. {list(bad.items())[:3]}"


def test_batched_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.MimoHipError):
        BatchedHipEngine(0)
    lib = _lib.load()
    row_off = np.array([0, 2], dtype=np.int64)
    Z = np.zeros((2, 2))
    assert lib.mimo_upload_batched(None, Z.ctypes.data, row_off.ctypes.data, 1, 2) == _lib.E_INVALID
    assert lib.mimo_estep_batched(None, None, None, None, 1, 0, None, None) == _lib.E_INVALID


def _offline(B, D):
    """An engine object without a context: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D = None, B, D
    eng.row_off = np.zeros(B + 1, dtype=np.int64)
    return eng


def test_batched_engine_argument_validation():
    eng = _offline(2, 3)
    K = 4
    c, b, W = np.zeros((2, K)), np.zeros((2, K, 3)), np.zeros((2, K, 3, 3))
    bad = [(c[:1], b, W), (c, b[:1], W), (c, b[:, :, :2], W), (c, b, W[:, :, :2]), (c[0], b, W), (c, b[:, :3], W)]
    for args in bad:
        with pytest.raises(ValueError):
            eng._params(*args)
    assert eng._params(c, b, W)[3] == K
    with pytest.raises(ValueError):
        eng.upload([])
    with pytest.raises(ValueError):
        eng.upload([np.zeros((3, 2)), np.zeros((3, 3))])
    with pytest.raises(ValueError):
        eng.upload([np.zeros(3)])
