"""Generator of tests/golden/cdf_ladder_hp.npz: the CDF F_k = cum_k / cum_{K-1} and the bound relB_k of the label-draw tests
(tests/cdf_ladder.py) at (Dz, K, N) = (2, 8, 41), seed 0, for the orders rising-640, rising-700, flat and flat-off, computed with
mpmath at 50 digits from logits evaluated in rational arithmetic.  tests/test_cdf_ladder_cpu.py holds the longdouble reference of
the GPU tests against it.

    python tests/golden/make_cdf_ladder_golden.py        (needs mpmath; a few seconds)

Stored per order o (dashes as underscores) as float64 pairs hi + lo (hi the rounded value, lo the rounded remainder: ~106 bits):
    <o>_F_hi / _lo        F_kn TIMES 2^512 (`scale_log2`): the smallest are near 1e-304, where the low word would be subnormal
    <o>_relB_hi / _lo     relB_k(n) = sum_{j<=k} e_j term_j / cum_k + sum_j r_j term_j + u0 (2 K + 12),  term_j = u0 (2 |x_j| + 8)
Only the inputs' recipe is shared with the test module (cdf_ladder.problem); the logits, the exponentials and the sums are this
script's own, in exact or 50-digit arithmetic.  A switched-off component (c_k = -inf) has e = 0 exactly and no term."""
import os
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cdf_ladder as CL  # noqa: E402

D, K, N, SEED = 2, 8, 41, 0
OUT = os.path.join(HERE, "cdf_ladder_hp.npz")
SCALE_LOG2 = 512

mp.mp.dps = 50


def mpf(q):
    return mp.mpf(q.numerator) / mp.mpf(q.denominator)


def pair(v):
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def pairs(values, shape):
    hl = np.array([pair(v) for v in values])
    return hl[:, 0].reshape(shape), hl[:, 1].reshape(shape)


def main():
    blob = {"shape": np.array([D, K, N, SEED], dtype=np.int64), "scale_log2": np.int64(SCALE_LOG2)}
    scale, u0 = mp.mpf(2) ** SCALE_LOG2, mp.mpf(2) ** -53
    for order in CL.ORDERS:
        Z, c, b, W = CL.problem(D, K, N, order, SEED)
        on = [bool(np.isfinite(c[k])) for k in range(K)]
        Zq = [[Fraction(float(v)) for v in row] for row in Z]
        F = [[None] * N for _ in range(K)]
        relB = [[None] * N for _ in range(K)]
        for n in range(N):
            L = [Fraction(float(c[k])) + sum(Fraction(float(b[k, d])) * Zq[n][d] for d in range(D))
                 - sum(Zq[n][d] * Fraction(float(W[k, d, e])) * Zq[n][e] for d in range(D) for e in range(D)) / 2
                 if on[k] else None for k in range(K)]
            m = max(l for l in L if l is not None)
            x = [mpf(l - m) if l is not None else None for l in L]
            e = [mp.exp(v) if v is not None else mp.mpf(0) for v in x]
            term = [u0 * (2 * abs(v) + 8) if v is not None else mp.mpf(0) for v in x]
            tot = mp.fsum(e)
            mean = mp.fsum(ej * tj for ej, tj in zip(e, term)) / tot
            for k in range(K):
                cum = mp.fsum(e[:k + 1])
                F[k][n] = cum / tot
                own = mp.fsum(ej * tj for ej, tj in zip(e[:k + 1], term[:k + 1])) / cum if cum > 0 else mp.mpf(0)
                relB[k][n] = own + mean + u0 * (2 * K + 12)
        t = order.replace("-", "_") + "_"
        blob[t + "F_hi"], blob[t + "F_lo"] = pairs([F[k][n] * scale for k in range(K) for n in range(N)], (K, N))
        blob[t + "relB_hi"], blob[t + "relB_lo"] = pairs([relB[k][n] for k in range(K) for n in range(N)], (K, N))
        print(f"{order}: smallest positive F {float(min(v for row in F for v in row if v > 0)):.3e}, "
              f"largest relB {float(max(max(row) for row in relB)):.3e}", flush=True)
    np.savez_compressed(OUT, **blob)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes")
    assert size < os.path.getsize(os.path.join(HERE, "softmax_ladder_hp.npz"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
