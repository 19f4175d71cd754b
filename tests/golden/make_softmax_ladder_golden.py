"""Generator of tests/golden/softmax_ladder_hp.npz: the softmax and the statistics of the ladder problem (tests/softmax_ladder.py)
at (Dz, K, N) = (2, 8, 257), seed 0, tops 640 and 700, computed with mpmath at 50 digits from logits evaluated in rational
arithmetic.  tests/test_softmax_ladder_cpu.py holds the longdouble reference of the GPU accuracy tests against it.

    python tests/golden/make_softmax_ladder_golden.py        (needs mpmath; a few seconds)

Stored per top t as float64 pairs hi + lo (hi the rounded value, lo the rounded remainder: ~106 bits):
    t<top>_lse_hi / _lo                       lse_n = log sum_k exp(L_kn)
    t<top>_R_hi / _lo, _n_, _sx_, _sxx_       r_kn, n_k = sum_n r_kn, sum_n r_kn z_n, sum_n r_kn z_n z_n' — each TIMES 2^512 (`scale`):
                                              the smallest of them are near 1e-305, where the low word would be subnormal
Only the inputs' recipe is shared with the test module (softmax_ladder.problem: the rows are drawn from a seeded generator);
the logits, the softmax and the sums are this script's own, in exact or 50-digit arithmetic."""
import os
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import softmax_ladder as SL  # noqa: E402

D, K, N, SEED = 2, 8, 257, 0
OUT = os.path.join(HERE, "softmax_ladder_hp.npz")
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
    scale = mp.mpf(2) ** SCALE_LOG2
    for top in SL.TOPS:
        Z, c, b, W = SL.problem(D, K, N, top, SEED)
        Zq = [[Fraction(float(v)) for v in row] for row in Z]
        L = [[Fraction(float(c[k])) + sum(Fraction(float(b[k, d])) * Zq[n][d] for d in range(D))
              - sum(Zq[n][d] * Fraction(float(W[k, d, e])) * Zq[n][e] for d in range(D) for e in range(D)) / 2
              for n in range(N)] for k in range(K)]
        R = [[None] * N for _ in range(K)]
        lse = []
        for n in range(N):
            m = max(L[k][n] for k in range(K))
            e = [mp.exp(mpf(L[k][n] - m)) for k in range(K)]
            tot = mp.fsum(e)
            lse.append(mpf(m) + mp.log(tot))
            for k in range(K):
                R[k][n] = e[k] / tot
        Zm = [[mpf(v) for v in row] for row in Zq]
        n_k = [mp.fsum(R[k]) for k in range(K)]
        sx = [mp.fsum(R[k][n] * Zm[n][d] for n in range(N)) for k in range(K) for d in range(D)]
        sxx = [mp.fsum(R[k][n] * Zm[n][d] * Zm[n][e] for n in range(N)) for k in range(K) for d in range(D) for e in range(D)]
        t = f"t{top}_"
        blob[t + "lse_hi"], blob[t + "lse_lo"] = pairs(lse, (N,))
        blob[t + "R_hi"], blob[t + "R_lo"] = pairs([R[k][n] * scale for k in range(K) for n in range(N)], (K, N))
        blob[t + "n_hi"], blob[t + "n_lo"] = pairs([v * scale for v in n_k], (K,))
        blob[t + "sx_hi"], blob[t + "sx_lo"] = pairs([v * scale for v in sx], (K, D))
        blob[t + "sxx_hi"], blob[t + "sxx_lo"] = pairs([v * scale for v in sxx], (K, D, D))
        print(f"top {top}: smallest r {float(min(min(r) for r in R)):.3e}, smallest n_k {float(min(n_k)):.3e}", flush=True)
    np.savez_compressed(OUT, **blob)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes")
    assert size < 200 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
