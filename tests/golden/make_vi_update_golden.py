"""Generator of tests/golden/vi_update_hp.npz: inputs and 50-digit values of one device-resident VI update (mimo_vi_run_batched,
one iteration) — the conjugate update of B mixtures of Gaussians with Dirichlet gating and untied Normal-Wishart components,
every output block of BatchedHipEngine.vi_state computed with mpmath at 50 digits and rounded to float64.  Its own code: the
formulas are those of the Normal-Wishart / Dirichlet conjugate update as include/mimo_hip.h states them for
mimo_host_gmm_vi_sweep / mimo_host_gmm_vi_bound.

    python tests/golden/make_vi_update_golden.py        (needs mpmath; about a minute)

What is stored, and why so little of it (the file stays under 200 KB):
  * rows and weight tables are small dyadic numbers (rows: multiples of 1/8 in [-4, 4] as int8; weights: multiples of 1/16 as
    uint8), so the statistics n_k, sum r z, sum r z z' are exact in float64 in ANY summation order — what the device's table pass
    returns is the exact statistic, bit for bit, and tests/vi_update_fixture.py rebuilds it with plain NumPy sums;
  * the priors are stored in standard form with dyadic m0, kappa0, alpha0 and a dyadic psi0^-1 per problem; the natural
    parameters the entry points take (pa = kappa0 m0, pb = kappa0, pc = psi0^-1 + kappa0 m0 m0', pd = nu0 - Dz = 2) are
    rebuilt from them with single float64 operations, which this script mirrors to define the inputs; prior_logZ is stored;
  * alpha, qa, qb, qc, qd and nus are single float64 additions of exact inputs, i.e. the correctly rounded exact values: the
    script asserts that against mpmath and the fixture module recomputes them;
  * psis and W are symmetric: their upper triangles are stored;
  * the problem without rows uses one prior for all its components (its posterior is its prior), so its blocks repeat and
    compress away.
Row counts per problem: 40, 0, 3 (two problems: 40, 0; one: 40).  The script asserts that every block C = qc - qb m m' has a
condition number <= 1e4.  For the two terms of the bound — differences of large quantities, exactly 0 where posterior = prior —
the sum of the absolute values of their summands is stored as the scale of the error metric."""
import os
import sys

import mpmath as mp
import numpy as np

SHAPES = [(3, 1, 1), (3, 2, 4), (2, 3, 17), (2, 16, 5), (2, 12, 33), (1, 7, 128)]       # (B, Dz, K)
ROWS = {3: (40, 0, 3), 2: (40, 0), 1: (40,)}
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vi_update_hp.npz")

mp.mp.dps = 50


def inputs(B, D, K, rng):
    """-> dict of the stored inputs of one shape."""
    rows = ROWS[B]
    Z, T = [], []
    m0, kappa0 = np.zeros((B, K, D)), np.zeros((B, K))
    psi0inv, alpha0 = np.zeros((B, D, D)), np.zeros((B, K))
    for b, n in enumerate(rows):
        centres = rng.integers(-20, 21, size=(K, D))
        lab = rng.integers(0, K, size=n)
        z = np.clip(centres[lab] + rng.integers(-6, 7, size=(n, D)), -32, 32).astype(np.int8)        # eighths
        r = rng.random((K, n)) ** 3 + 4.0 * (np.arange(K)[:, None] == lab[None, :])
        r /= r.sum(axis=0, keepdims=True) if n else 1.0
        Z.append(z)
        T.append(np.rint(16.0 * r).astype(np.uint8))                                              # sixteenths
        G = rng.integers(-4, 5, size=(D, D)) / 4.0
        psi0inv[b] = (G @ G.T) / 4.0 + np.eye(D) * (1.0 + 0.25 * b)                              # dyadic, exact
        if n == 0:
            kappa0[b], alpha0[b] = 0.5, 1.5                                                      # one prior for all k
        else:
            m0[b] = rng.integers(-8, 9, size=(K, D)) / 4.0
            kappa0[b] = rng.integers(1, 9, size=K) / 8.0
            alpha0[b] = rng.integers(1, 7, size=K) / 2.0
    return dict(rows=np.array(rows, dtype=np.int64), Z=np.concatenate(Z).reshape(-1, D),
                T=np.concatenate([t.reshape(-1) for t in T]) if sum(rows) else np.zeros(0, dtype=np.uint8),
                m0=m0, kappa0=kappa0, psi0inv=psi0inv, alpha0=alpha0)


def mpm(a):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])


def logdet_spd(A, D):
    L = mp.cholesky(A)
    return 2 * sum(mp.log(L[i, i]) for i in range(D))


def ln_multigamma(x, D):
    return mp.mpf(D * (D - 1)) / 4 * mp.log(mp.pi) + sum(mp.loggamma(x - mp.mpf(j) / 2) for j in range(D))


def nw_log_partition(kappa, nu, half_logdet_psi, D):
    return -mp.mpf(D) / 2 * mp.log(kappa) + (nu * D / 2 * mp.log(2) + ln_multigamma(nu / 2, D) + nu * half_logdet_psi)


def shape_values(B, D, K, g):
    """-> (prior_logZ (B, K), dict of the high-precision output blocks) of one shape."""
    f = lambda v: mp.mpf(float(v))
    tri = np.triu_indices(D)
    out = {k: np.zeros((B, K)) for k in ("hld", "cc", "E2", "E4", "elp", "c_total")}
    out.update(mus=np.zeros((B, K, D)), bb=np.zeros((B, K, D)), psis_tri=np.zeros((B, K, len(tri[0]))),
               W_tri=np.zeros((B, K, len(tri[0]))), vlb=np.zeros((B, 2)), vlb_scale=np.zeros((B, 2)))
    plz = np.zeros((B, K))
    log_base = -mp.mpf(D) / 2 * mp.log(2 * mp.pi)
    zo = to = 0
    worst = 0.0
    for b in range(B):
        n = int(g["rows"][b])
        z = g["Z"][zo:zo + n].astype(np.float64) / 8.0
        r = g["T"][to:to + K * n].reshape(K, n).astype(np.float64) / 16.0
        zo, to = zo + n, to + K * n
        # exact statistics (dyadic inputs: float64 sums are exact), checked against mpmath for one entry per component below
        sn, sx, sxx = r.sum(axis=1), r @ z, np.einsum('kn,na,nb->kab', r, z, z)
        P0 = mpm(g["psi0inv"][b])
        hld0 = -logdet_spd(P0, D) / 2                          # 1/2 log det psi0
        nu0 = mp.mpf(D + 2)
        alpha = [f(g["alpha0"][b, k]) + f(sn[k]) for k in range(K)]
        s, s0 = sum(alpha), sum(f(v) for v in g["alpha0"][b])
        terms, scales = [], []
        for k in range(K):
            kap0, mk0 = f(g["kappa0"][b, k]), mpm(g["m0"][b, k]).T
            # the inputs as the entry point receives them: single float64 operations on exact numbers
            pa64 = g["kappa0"][b, k] * g["m0"][b, k]
            pc64 = g["psi0inv"][b] + g["kappa0"][b, k] * np.outer(g["m0"][b, k], g["m0"][b, k])
            assert mpm(pc64) == P0 + kap0 * mk0 * mk0.T and mpm(pa64).T == kap0 * mk0, "the prior's natural parameters are not exact"
            plz[b, k] = float(nw_log_partition(kap0, nu0, hld0, D))
            qa, qb, qd = mpm(pa64).T + mpm(sx[k]).T, kap0 + f(sn[k]), mp.mpf(2) + f(sn[k])
            qc = mpm(pc64) + mpm(sxx[k])
            for exact, single in ((qa, pa64 + sx[k]), (qc, pc64 + sxx[k])):
                assert np.array_equal(np.array(exact.tolist(), dtype=np.float64).reshape(np.shape(single)), single)
            assert float(qb) == g["kappa0"][b, k] + sn[k] and float(qd) == 2.0 + sn[k] and float(alpha[k]) == g["alpha0"][b, k] + sn[k]
            m = qa / qb
            C = qc - qb * m * m.T
            worst = max(worst, float(np.linalg.cond(np.array(C.tolist(), dtype=np.float64))))
            psi = C ** -1
            hld = -logdet_spd(C, D) / 2
            nu = qd + D
            assert float(nu) == 2.0 + sn[k] + D
            W = nu * psi
            bb = W * m
            E2 = -(D / qb + (m.T * bb)[0]) / 2
            E4 = (sum(mp.digamma((nu - i) / 2) for i in range(D)) + D * mp.log(2) + 2 * hld) / 2
            cc = log_base + E2 + E4
            elp = mp.digamma(alpha[k]) - mp.digamma(s)
            logZq = nw_log_partition(qb, nu, hld, D)
            ddot = lambda A, Bm: sum(A[i, j] * Bm[i, j] for i in range(D) for j in range(D))
            pa, pcm = mpm(pa64).T, mpm(pc64)
            iq = (qa.T * bb)[0] + qb * E2 - ddot(qc, W) / 2 + qd * E4
            ip = (pa.T * bb)[0] + kap0 * E2 - ddot(pcm, W) / 2 + mp.mpf(2) * E4
            pz = f(plz[b, k])                                   # the rounded log-partition: it is an input
            terms.append((logZq - log_base - iq) - (pz - log_base - ip))
            scales.append(abs(logZq) + abs(iq) + abs(pz) + abs(ip) + 2 * abs(log_base))
            for name, v in (("hld", hld), ("cc", cc), ("E2", E2), ("E4", E4), ("elp", elp), ("c_total", cc + elp)):
                out[name][b, k] = float(v)
            out["mus"][b, k] = [float(v) for v in m]
            out["bb"][b, k] = [float(v) for v in bb]
            out["psis_tri"][b, k] = [float(psi[i, j]) for i, j in zip(*tri)]
            out["W_tri"][b, k] = [float(W[i, j]) for i, j in zip(*tri)]
        a0 = [f(v) for v in g["alpha0"][b]]
        elps = [mp.digamma(alpha[k]) - mp.digamma(s) for k in range(K)]
        lq, lp = sum(mp.loggamma(v) for v in alpha), sum(mp.loggamma(v) for v in a0)
        iq = sum((alpha[k] - 1) * elps[k] for k in range(K))
        ip = sum((a0[k] - 1) * elps[k] for k in range(K))
        out["vlb"][b] = [float(((lq - mp.loggamma(s)) - iq) - ((lp - mp.loggamma(s0)) - ip)), float(sum(terms))]
        out["vlb_scale"][b] = [float(abs(lq) + abs(mp.loggamma(s)) + abs(iq) + abs(lp) + abs(mp.loggamma(s0)) + abs(ip)),
                               float(sum(scales))]
    assert worst <= 1e4, f"condition number {worst:.3g} > 1e4"
    return plz, out, worst


def main():
    rng = np.random.default_rng(20240611)
    blob = {"shapes": np.array(SHAPES, dtype=np.int64)}
    for idx, (B, D, K) in enumerate(SHAPES):
        g = inputs(B, D, K, rng)
        plz, hp, worst = shape_values(B, D, K, g)
        print(f"shape {idx}: B={B} Dz={D} K={K}  worst condition number {worst:.3g}", flush=True)
        for name, v in g.items():
            blob[f"s{idx}_{name}"] = v
        blob[f"s{idx}_plz"] = plz
        for name, v in hp.items():
            blob[f"s{idx}_hp_{name}"] = v
    np.savez_compressed(OUT, **blob)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes")
    assert size < 200 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
