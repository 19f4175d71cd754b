"""Diagnostic: time of mimo_host_block_order at K = 64, D = 16 (one core; 64, 51 and 40 of the components with mass), next to a
ctypes call that does nothing (profiles/r13_c2_block_order.txt; tools/host_pool_time.py has the sweep's other host calls).
    python tools/block_order_time.py"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mimo_amd import _lib
lib = _lib.load()
rng = np.random.default_rng(0)
K, D = 64, 16
for frac in (0.0, 0.15, 0.4):
    centres = rng.normal(0, 6, size=(32, D))
    means = np.ascontiguousarray(centres[rng.integers(32, size=K)] + 0.05 * rng.standard_normal((K, D)))
    mass = np.where(rng.random(K) < frac, 1e-2, 100 + 1000 * rng.random(K))
    order = np.empty(K, dtype=np.int32)
    m, w, o = means.ctypes.data, mass.ctypes.data, order.ctypes.data
    best = 1e9
    for rep in range(5):
        t0 = time.perf_counter()
        for _ in range(5000):
            lib.mimo_host_block_order(K, D, m, w, 16, o)
        best = min(best, (time.perf_counter() - t0) / 5000)
    print("mimo_host_block_order K=64 D=16, %d active: %.2f us per call" % (int((mass >= 1).sum()), best * 1e6))
t0 = time.perf_counter()
for _ in range(20000):
    lib.mimo_host_digamma(1.0)
print("empty ctypes call %.2f us" % ((time.perf_counter() - t0) / 20000 * 1e6))
