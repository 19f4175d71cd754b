"""Generator of tests/golden/vi_ilr_update_hp.npz: inputs and 50-digit values of one device-resident VI update of B mixtures of
linear-Gaussian experts (mimo_vi_ilr_run_batched, one iteration) — the conjugate update of the basis (Normal-Wishart over x), of
the affine experts (matrix-normal-Wishart of y | [x, 1]) and of the gating (Dirichlet or truncated stick-breaking), the joint
canonical form over z = [x, y] and the three terms of the bound, computed with mpmath at 50 digits and rounded to float64.  Its
own code: the formulas are those include/mimo_hip.h states for mimo_vi_ilr_run_batched.

    python tests/golden/make_vi_ilr_update_golden.py        (needs mpmath; a few minutes)

What is stored (the file stays under 200 KB), on the pattern of make_vi_update_golden.py:
  * rows z = [x, y] are multiples of 1/8 (int8), weight tables multiples of 1/16 (uint8): the joint statistics n, sum r z,
    sum r z z' are exact in float64 in any summation order, so the device's table pass returns the exact statistic and
    tests/vi_ilr_update_fixture.py rebuilds it with plain NumPy sums;
  * priors in standard form, dyadic: the gating's alpha0 or (gamma0, delta0); the basis' m0, kappa0 and one psi0^-1 per problem
    (nu0 = dx + 2); the experts' M0, one K0 and one psi0^-1 per problem (nu0 = dy + 2).  The natural parameters the entry point
    takes are rebuilt from them with float64 operations that are exact on these numbers (asserted here against mpmath); the two
    log-partition blocks are stored;
  * the natural parameters of the posterior, the gating's posterior parameters and both nus are single float64 additions of exact
    inputs: the fixture module recomputes them;
  * symmetric blocks as upper triangles; the experts' own (b, W) over z are rearrangements of E1, E2 and nu psi and are not stored;
  * the problem without rows uses one prior for all its components: its blocks repeat and compress away.
Row counts per problem: 40, 0, 3.  The script asserts a condition number <= 1e4 for the three factorised blocks of every
component: the basis' C = qc - qb m m', Kq, and the experts' C = c - a Kq^-1 a'.  For each of the three terms of the bound the sum of
the absolute values of its summands is stored as the error scale of the problem without rows (where the term is exactly 0)."""
import os
import sys

import mpmath as mp
import numpy as np

# (B, dx, dy, K, gating: 0 Dirichlet, 1 stick-breaking)
SHAPES = [(3, 1, 1, 1, 0), (3, 1, 1, 6, 0), (2, 2, 1, 17, 1), (2, 8, 4, 5, 1), (2, 15, 1, 2, 0), (2, 1, 15, 3, 1), (2, 1, 3, 33, 0),
          (1, 1, 1, 128, 1)]
ROWS = {3: (40, 0, 3), 2: (40, 0), 1: (40,)}
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vi_ilr_update_hp.npz")

mp.mp.dps = 50


def spd_dyadic(rng, n, shift):
    G = rng.integers(-4, 5, size=(n, n)) / 4.0
    return (G @ G.T) / 4.0 + np.eye(n) * shift


def inputs(B, dx, dy, K, stick, rng):
    """-> dict of the stored inputs of one shape."""
    rows, D, dc = ROWS[B], dx + dy, dx + 1
    Z, T = [], []
    g0, g1 = np.zeros((B, K)), np.zeros((B, K))
    bm0, bkappa0, bpsi0inv = np.zeros((B, K, dx)), np.zeros((B, K)), np.zeros((B, dx, dx))
    M0, K0, ypsi0inv = np.zeros((B, K, dy, dc)), np.zeros((B, dc, dc)), np.zeros((B, dy, dy))
    for b, n in enumerate(rows):
        centres = rng.integers(-20, 21, size=(K, D))
        lab = rng.integers(0, K, size=n)
        z = np.clip(centres[lab] + rng.integers(-6, 7, size=(n, D)), -32, 32).astype(np.int8)        # eighths
        r = rng.random((K, n)) ** 3 + 4.0 * (np.arange(K)[:, None] == lab[None, :])
        r /= r.sum(axis=0, keepdims=True) if n else 1.0
        Z.append(z)
        T.append(np.rint(16.0 * r).astype(np.uint8))                                              # sixteenths
        bpsi0inv[b] = spd_dyadic(rng, dx, 1.0 + 0.25 * b)
        K0[b] = spd_dyadic(rng, dc, 2.0 + 0.5 * b)
        ypsi0inv[b] = spd_dyadic(rng, dy, 1.0 + 0.25 * b)
        if n == 0:                                                                                # one prior for all k
            bkappa0[b] = 0.5
            g0[b], g1[b] = (1.0, 2.5) if stick else (1.5, 0.0)
            M0[b] = rng.integers(-4, 5, size=(dy, dc)) / 4.0
        else:
            bm0[b] = rng.integers(-8, 9, size=(K, dx)) / 4.0
            bkappa0[b] = rng.integers(1, 9, size=K) / 8.0
            M0[b] = rng.integers(-4, 5, size=(K, dy, dc)) / 4.0
            if stick:
                g0[b], g1[b] = rng.integers(2, 7, size=K) / 2.0, rng.integers(2, 13, size=K) / 2.0
            else:
                g0[b] = rng.integers(1, 7, size=K) / 2.0
    return dict(rows=np.array(rows, dtype=np.int64), Z=np.concatenate(Z).reshape(-1, D),
                T=np.concatenate([t.reshape(-1) for t in T]) if sum(rows) else np.zeros(0, dtype=np.uint8),
                g0=g0, g1=g1, bm0=bm0, bkappa0=bkappa0, bpsi0inv=bpsi0inv, M0=M0, K0=K0, ypsi0inv=ypsi0inv)


def mpm(a):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])


def f64(A):
    return np.array(A.tolist(), dtype=np.float64)


def logdet_spd(A):
    L = mp.cholesky(A)
    return 2 * sum(mp.log(L[i, i]) for i in range(A.rows))


def ln_multigamma(x, D):
    return mp.mpf(D * (D - 1)) / 4 * mp.log(mp.pi) + sum(mp.loggamma(x - mp.mpf(j) / 2) for j in range(D))


def wishart_log_partition(nu, half_logdet_psi, D):
    return nu * D / 2 * mp.log(2) + ln_multigamma(nu / 2, D) + nu * half_logdet_psi


def ddot(A, Bm):
    return sum(A[i, j] * Bm[i, j] for i in range(A.rows) for j in range(A.cols))


def adot(A, Bm):
    return sum(abs(A[i, j] * Bm[i, j]) for i in range(A.rows) for j in range(A.cols))


def cond(A):
    return float(np.linalg.cond(f64(A)))


def shape_values(B, dx, dy, K, stick, g):
    """-> (basis log Z (B, K), experts log Z (B, K), dict of the high-precision output blocks, worst condition number)."""
    f = lambda v: mp.mpf(float(v))
    D, dc = dx + dy, dx + 1
    tx, tc, ty, tz = np.triu_indices(dx), np.triu_indices(dc), np.triu_indices(dy), np.triu_indices(D)
    out = {k: np.zeros((B, K)) for k in ("hld", "cc", "E2", "E4", "m_hld", "m_cc", "m_E4", "e_log_pi", "c_total")}
    out.update(mus=np.zeros((B, K, dx)), bb=np.zeros((B, K, dx)), psis_tri=np.zeros((B, K, len(tx[0]))),
               W_tri=np.zeros((B, K, len(tx[0]))), m_Ms=np.zeros((B, K, dy, dc)), m_psis_tri=np.zeros((B, K, len(ty[0]))),
               m_Kinv_tri=np.zeros((B, K, len(tc[0]))), m_E1=np.zeros((B, K, dy, dc)), m_E2_tri=np.zeros((B, K, len(tc[0]))),
               j_bb=np.zeros((B, K, D)), j_W_tri=np.zeros((B, K, len(tz[0]))), vlb=np.zeros((B, 3)), vlb_scale=np.zeros((B, 3)))
    plz, mlz = np.zeros((B, K)), np.zeros((B, K))
    lb1 = -mp.mpf(dx) / 2 * mp.log(2 * mp.pi)
    lb2 = -mp.mpf(dy * dc) / 2 * mp.log(2 * mp.pi)
    zo = to = 0
    worst = 0.0
    for b in range(B):
        n = int(g["rows"][b])
        z = g["Z"][zo:zo + n].astype(np.float64) / 8.0
        r = g["T"][to:to + K * n].reshape(K, n).astype(np.float64) / 16.0
        zo, to = zo + n, to + K * n
        sn, sz, szz = r.sum(axis=1), r @ z, np.einsum('kn,na,nb->kab', r, z, z)      # exact (dyadic inputs)
        # ---- gating ----
        cnt = [f(v) for v in sn]
        if stick:
            acc = [sum(cnt[k + 1:], mp.mpf(0)) for k in range(K)]
            gam = [f(g["g0"][b, k]) + cnt[k] for k in range(K)]
            dlt = [f(g["g1"][b, k]) + acc[k] for k in range(K)]
            gam0, dlt0 = [f(v) for v in g["g0"][b]], [f(v) for v in g["g1"][b]]
            for k in range(K):      # single float64 additions of exact numbers
                assert float(acc[k]) == float(np.sum(sn[k + 1:])) and float(gam[k]) == g["g0"][b, k] + sn[k]
                assert float(dlt[k]) == g["g1"][b, k] + float(acc[k])
            es = [mp.digamma(gam[k]) - mp.digamma(gam[k] + dlt[k]) for k in range(K)]
            er = [mp.digamma(dlt[k]) - mp.digamma(gam[k] + dlt[k]) for k in range(K)]
            elp = [es[k] + sum(er[:k], mp.mpf(0)) for k in range(K)]
            betaln = lambda x, y: mp.loggamma(x) + mp.loggamma(y) - mp.loggamma(x + y)
            lq = sum(betaln(gam[k], dlt[k]) for k in range(K))
            lp = sum(betaln(gam0[k], dlt0[k]) for k in range(K))
            iq = sum((gam[k] - 1) * es[k] + (dlt[k] - 1) * er[k] for k in range(K))
            ip = sum((gam0[k] - 1) * es[k] + (dlt0[k] - 1) * er[k] for k in range(K))
            gate = (lq - iq) - (lp - ip)
            gscale = sum(abs(mp.loggamma(gam[k])) + abs(mp.loggamma(dlt[k])) + abs(mp.loggamma(gam[k] + dlt[k]))
                         + abs(mp.loggamma(gam0[k])) + abs(mp.loggamma(dlt0[k])) + abs(mp.loggamma(gam0[k] + dlt0[k]))
                         + abs((gam[k] - 1) * es[k]) + abs((dlt[k] - 1) * er[k]) + abs((gam0[k] - 1) * es[k])
                         + abs((dlt0[k] - 1) * er[k]) for k in range(K))
        else:
            al = [f(g["g0"][b, k]) + cnt[k] for k in range(K)]
            a0 = [f(v) for v in g["g0"][b]]
            for k in range(K):
                assert float(al[k]) == ((g["g0"][b, k] - 1.0) + sn[k]) + 1.0
            s, s0 = sum(al), sum(a0)
            elp = [mp.digamma(al[k]) - mp.digamma(s) for k in range(K)]
            lq, lp = sum(mp.loggamma(v) for v in al), sum(mp.loggamma(v) for v in a0)
            iq = sum((al[k] - 1) * elp[k] for k in range(K))
            ip = sum((a0[k] - 1) * elp[k] for k in range(K))
            gate = ((lq - mp.loggamma(s)) - iq) - ((lp - mp.loggamma(s0)) - ip)
            gscale = sum(abs(mp.loggamma(v)) for v in al) + sum(abs(mp.loggamma(v)) for v in a0) + abs(mp.loggamma(s))\
                + abs(mp.loggamma(s0)) + sum(abs((al[k] - 1) * elp[k]) + abs((a0[k] - 1) * elp[k]) for k in range(K))
        # ---- the priors' shared factors ----
        P0 = mpm(g["bpsi0inv"][b])
        bhld0 = -logdet_spd(P0) / 2
        K0m, Y0 = mpm(g["K0"][b]), mpm(g["ypsi0inv"][b])
        ld_K0, yhld0 = logdet_spd(K0m), -logdet_spd(Y0) / 2
        terms1, scales1, terms2, scales2 = [], [], [], []
        for k in range(K):
            # ---- basis: Normal-Wishart over x ----
            kap0, mk0 = f(g["bkappa0"][b, k]), mpm(g["bm0"][b, k]).T
            pa64 = g["bkappa0"][b, k] * g["bm0"][b, k]
            pc64 = g["bpsi0inv"][b] + g["bkappa0"][b, k] * np.outer(g["bm0"][b, k], g["bm0"][b, k])
            assert mpm(pc64) == P0 + kap0 * mk0 * mk0.T and mpm(pa64).T == kap0 * mk0, "the basis' natural parameters are not exact"
            nu0 = mp.mpf(dx + 2)
            plz[b, k] = float(-mp.mpf(dx) / 2 * mp.log(kap0) + wishart_log_partition(nu0, bhld0, dx))
            sx, sxx = sz[k, :dx], szz[k, :dx, :dx]
            qa, qb, qd = mpm(pa64).T + mpm(sx).T, kap0 + cnt[k], mp.mpf(2) + cnt[k]
            qc = mpm(pc64) + mpm(sxx)
            m = qa / qb
            C = qc - qb * m * m.T
            worst = max(worst, cond(C))
            psi = C ** -1
            hld = -logdet_spd(C) / 2
            nu = qd + dx
            W1 = nu * psi
            b1 = W1 * m
            E2 = -(dx / qb + (m.T * b1)[0]) / 2
            E4 = (sum(mp.digamma((nu - i) / 2) for i in range(dx)) + dx * mp.log(2) + 2 * hld) / 2
            cc1 = lb1 + E2 + E4
            logZq = -mp.mpf(dx) / 2 * mp.log(qb) + wishart_log_partition(nu, hld, dx)
            pa, pcm, pz = mpm(pa64).T, mpm(pc64), f(plz[b, k])
            iq = (qa.T * b1)[0] + qb * E2 - ddot(qc, W1) / 2 + qd * E4
            ip = (pa.T * b1)[0] + kap0 * E2 - ddot(pcm, W1) / 2 + mp.mpf(2) * E4
            terms1.append((logZq - lb1 - iq) - (pz - lb1 - ip))
            scales1.append(abs(logZq) + abs(pz) + 2 * abs(lb1) + sum(abs(qa[i] * b1[i]) + abs(pa[i] * b1[i]) for i in range(dx))
                           + abs(qb * E2) + abs(kap0 * E2) + (adot(qc, W1) + adot(pcm, W1)) / 2 + abs(qd * E4) + abs(2 * E4))
            # ---- experts: matrix-normal-Wishart of y | x~ ----
            M0m = mpm(g["M0"][b, k])
            ma64 = g["M0"][b, k] @ g["K0"][b]
            mc64 = g["ypsi0inv"][b] + ma64 @ g["M0"][b, k].T
            assert mpm(ma64) == M0m * K0m and mpm(mc64) == Y0 + M0m * K0m * M0m.T, "the experts' natural parameters are not exact"
            nu0y = mp.mpf(dy + 2)
            md = nu0y - dy - 1 + dc
            mlz[b, k] = float(-mp.mpf(dy) / 2 * ld_K0 + wishart_log_partition(nu0y, yhld0, dy))
            syx = np.concatenate([szz[k, dx:, :dx], sz[k, dx:, None]], axis=1)
            sxt = np.block([[szz[k, :dx, :dx], sz[k, :dx, None]], [sz[k, None, :dx], np.array([[sn[k]]])]])
            a = mpm(ma64) + mpm(syx)
            Kq = K0m + mpm(sxt)
            c = mpm(mc64) + mpm(szz[k, dx:, dx:])
            d = md + cnt[k]
            worst = max(worst, cond(Kq))
            Ki = Kq ** -1
            M = a * Ki
            Cm = c - a * M.T
            worst = max(worst, cond(Cm))
            psiy = Cm ** -1
            hld2 = -logdet_spd(Cm) / 2
            nu2 = d + dy + 1 - dc
            E1 = nu2 * psiy * M
            E2m = -(dy * Ki + M.T * E1) / 2
            E3m = -nu2 * psiy / 2
            E4m = (sum(mp.digamma((nu2 - i) / 2) for i in range(dy)) + dy * mp.log(2) + 2 * hld2) / 2
            cc2 = -mp.mpf(dy) / 2 * mp.log(2 * mp.pi) + E4m + E2m[dx, dx]
            logZqm = -mp.mpf(dy) / 2 * logdet_spd(Kq) + wishart_log_partition(nu2, hld2, dy)
            mam, mcm, mz = mpm(ma64), mpm(mc64), f(mlz[b, k])
            iqm = ddot(a, E1) + ddot(Kq, E2m) + ddot(c, E3m) + d * E4m
            ipm = ddot(mam, E1) + ddot(K0m, E2m) + ddot(mcm, E3m) + md * E4m
            terms2.append((logZqm - lb2 - iqm) - (mz - lb2 - ipm))
            scales2.append(abs(logZqm) + abs(mz) + 2 * abs(lb2) + adot(a, E1) + adot(mam, E1) + adot(Kq, E2m) + adot(K0m, E2m)
                           + adot(c, E3m) + adot(mcm, E3m) + abs(d * E4m) + abs(md * E4m))
            # ---- the joint canonical form over z ----
            Wj = mp.zeros(D, D)
            bj = [mp.mpf(0)] * D
            for i in range(dx):
                for j in range(dx):
                    Wj[i, j] = -2 * E2m[i, j] + W1[i, j]
                bj[i] = 2 * E2m[i, dx] + b1[i]
            for i in range(dy):
                for j in range(dy):
                    Wj[dx + i, dx + j] = nu2 * psiy[i, j]
                for j in range(dx):
                    Wj[dx + i, j] = Wj[j, dx + i] = -E1[i, j]
                bj[dx + i] = E1[i, dx]
            for name, v in (("hld", hld), ("cc", cc1), ("E2", E2), ("E4", E4), ("m_hld", hld2), ("m_cc", cc2), ("m_E4", E4m),
                            ("e_log_pi", elp[k]), ("c_total", cc1 + cc2 + elp[k])):
                out[name][b, k] = float(v)
            out["mus"][b, k] = [float(v) for v in m]
            out["bb"][b, k] = [float(v) for v in b1]
            out["psis_tri"][b, k] = [float(psi[i, j]) for i, j in zip(*tx)]
            out["W_tri"][b, k] = [float(W1[i, j]) for i, j in zip(*tx)]
            out["m_Ms"][b, k] = f64(M)
            out["m_E1"][b, k] = f64(E1)
            out["m_psis_tri"][b, k] = [float(psiy[i, j]) for i, j in zip(*ty)]
            out["m_Kinv_tri"][b, k] = [float(Ki[i, j]) for i, j in zip(*tc)]
            out["m_E2_tri"][b, k] = [float(E2m[i, j]) for i, j in zip(*tc)]
            out["j_bb"][b, k] = [float(v) for v in bj]
            out["j_W_tri"][b, k] = [float(Wj[i, j]) for i, j in zip(*tz)]
        out["vlb"][b] = [float(gate), float(sum(terms1)), float(sum(terms2))]
        out["vlb_scale"][b] = [float(gscale), float(sum(scales1)), float(sum(scales2))]
    assert worst <= 1e4, f"condition number {worst:.3g} > 1e4"
    return plz, mlz, out, worst


def main():
    rng = np.random.default_rng(20240917)
    blob = {"shapes": np.array(SHAPES, dtype=np.int64)}
    for idx, (B, dx, dy, K, stick) in enumerate(SHAPES):
        g = inputs(B, dx, dy, K, stick, rng)
        plz, mlz, hp, worst = shape_values(B, dx, dy, K, stick, g)
        print(f"shape {idx}: B={B} dx={dx} dy={dy} K={K} stick={stick}  worst condition number {worst:.3g}", flush=True)
        for name, v in g.items():
            blob[f"s{idx}_{name}"] = v
        blob[f"s{idx}_plz"], blob[f"s{idx}_mlz"] = plz, mlz
        for name, v in hp.items():
            blob[f"s{idx}_hp_{name}"] = v
    np.savez_compressed(OUT, **blob)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes")
    assert size < 200 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
