"""Diagnostic: time of mimo_host_estep_certificate at K = 64, D = 16 on one core (the method of tools/block_order_time.py), for a
reference compared with itself, a small move of every component, and a move that sends a few components down the grid
(profiles/r16_c2_estep_certificate.txt).  --cached: the form cert_plan uses from the second certified pass on — the reference block
made once (mimo_host_estep_certificate_ref, timed on its own), then mimo_host_estep_certificate_cur per call; the two forms' `out` and
`table` are compared byte for byte on the way (profiles/r17_c2_cert_check.txt).
    python tools/estep_certificate_time.py [--cached]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mimo_amd import _lib
lib = _lib.load()
rng = np.random.default_rng(0)
K, D = 64, 16


def canonical(mu, W, ch):
    b = np.einsum("kij,kj->ki", W, mu)
    return [np.ascontiguousarray(x) for x in (ch - 0.5 * np.einsum("kd,kd->k", b, mu), b, W)]


A = rng.standard_normal((K, D, D))
W0 = np.einsum("kij,klj->kil", A, A) / D + 0.3 * np.eye(D)
mu0, ch0 = rng.normal(0, 6, size=(K, D)), rng.normal(-20, 5, size=K)
ref = canonical(mu0, W0, ch0)
out, table = np.empty(5 * K + 4), np.empty(4 + 2 * K)
cached = "--cached" in sys.argv[1:]
if cached:
    block = np.empty(lib.mimo_host_estep_certificate_ref_size(K, D))
    rargs = [x.ctypes.data for x in ref]
    best = 1e9
    for rep in range(5):
        t0 = time.perf_counter()
        for _ in range(500):
            assert lib.mimo_host_estep_certificate_ref(K, D, *rargs, block.ctypes.data) == 0
        best = min(best, (time.perf_counter() - t0) / 500)
    print("mimo_host_estep_certificate_ref K=64 D=16 (%d doubles): %.1f us per call" % (block.size, best * 1e6))
for name, move, wild in (("itself", 0.0, 0), ("small move", 0.01, 0), ("small move, 6 components several-fold", 0.01, 6)):
    W = W0 * (1.0 + move * rng.uniform(-1, 1, size=(K, 1, 1)))
    W[:wild] *= rng.uniform(2.0, 8.0, size=(wild, 1, 1))
    cur = canonical(mu0 + move * rng.standard_normal((K, D)), W, ch0 + move)
    args = [x.ctypes.data for x in ref + cur]
    best = 1e9
    for rep in range(5):
        t0 = time.perf_counter()
        for _ in range(500):
            assert lib.mimo_host_estep_certificate(K, D, *args, -41.6, out.ctypes.data, table.ctypes.data) == 0
        best = min(best, (time.perf_counter() - t0) / 500)
    print("mimo_host_estep_certificate K=64 D=16, %s: %.1f us per call" % (name, best * 1e6))
    if cached:
        out2, table2 = np.empty_like(out), np.empty_like(table)
        cargs = [x.ctypes.data for x in cur]
        best = 1e9
        for rep in range(5):
            t0 = time.perf_counter()
            for _ in range(500):
                assert lib.mimo_host_estep_certificate_cur(K, D, block.ctypes.data, *cargs, -41.6, out2.ctypes.data, table2.ctypes.data) == 0
            best = min(best, (time.perf_counter() - t0) / 500)
        assert out2.tobytes() == out.tobytes() and table2.tobytes() == table.tobytes()
        print("mimo_host_estep_certificate_cur K=64 D=16, %s: %.1f us per call (same bytes)" % (name, best * 1e6))
