"""Per-row certificates of the fused mean-field E-step, on the CPU ("E-step certificates"): a row whose
log-densities an earlier ("reference") pass computed exactly is proven dead outside its row block for a later pass from how far
a Gaussian log-density can move in the component's own whitened coordinates.

  * the NumPy model of the bound, in two forms: with ONE set of constants over all components, and as built — the constants
    per class of components (two classes, split at the widest gap of the reference peaks), the positive parts kept, the square
    roots replaced by their affine bounds, the eigenvalues by the enclosure of mimo_host_estep_certificate;
  * soundness of both on every (row, component) of random posteriors under moves from nothing to several sigma;
  * mimo_host_estep_certificate against NumPy, its rejections, and a sanitizer run of a stand-alone program;
  * the model of what the certificates buy on the benchmark's own data recipe and start, under the refresh policy of the
    library: the share of proven rows and of (tile, wave) pairs that need at most 16 of their 32 rows.  With one set of
    constants the share is 0.00 (the go / no-go figure of the first form: no-go), as built 0.99."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mimo_amd import _lib
from test_block_order_cpu import block_order, blocks_of, partition, _log_densities, _packed_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LN_TAU, EPS = 32, -60 * np.log(2.0), 1e-3
RENEW = 16           # certified passes after which the library takes a new reference pass (kCertRenew, mimo_abi.cpp)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def peaks(c, b, W):
    """(mu_k, c^_k) of l_k(x) = c_k + b_k.x - x'W_k x / 2 = c^_k - |x - mu_k|^2_W / 2"""
    mu = np.linalg.solve(W, b[..., None])[..., 0]
    return mu, c + 0.5 * np.einsum("kd,kd->k", b, mu)


def constants(ref, cur):
    """c^0, c^, rho, rho_bar, d per component (exact eigenvalues) of the current (c, b, W) against the reference one"""
    mu0, ch0 = peaks(*ref)
    mu, ch = peaks(*cur)
    K = len(ch)
    rho, rho_bar, d = np.empty(K), np.empty(K), np.empty(K)
    for k in range(K):
        Lc = np.linalg.cholesky(ref[2][k])
        Li = np.linalg.inv(Lc)
        ev = np.linalg.eigvalsh(Li @ cur[2][k] @ Li.T)
        rho[k], rho_bar[k] = ev[0], ev[-1]
        d[k] = np.linalg.norm(Lc.T @ (mu[k] - mu0[k]))
    return ch0, ch, rho, rho_bar, d


def certificates(L0, blk):
    """(k*, m0, a0) of every row from the reference pass's log-densities L0 (K, N) and the block of every component: where the
    largest is, the largest, and the largest outside the row block of k* (a0 = m0 - g)"""
    ks = L0.argmax(axis=0)
    outside = np.where(blk[:, None] != blk[ks][None, :], L0, -np.inf)
    return ks, L0.max(axis=0), outside.max(axis=0)


def bounds_one_class(cert, consts):
    """(U_n, M_n) with one set of constants: no component outside the block of k*_n reaches U_n, the row's maximum is at least
    M_n.  U_n = +inf where the certificate says nothing (Q_n <= d_max^2)."""
    ks, m0, a0 = cert
    ch0, ch, rho, rho_bar, d = consts
    Q = 2.0 * (ch0.min() - a0)
    d_max = d.max()
    U = np.where(Q > d_max * d_max, ch.max() - 0.5 * rho.min() * (np.sqrt(np.maximum(Q, 0.0)) - d_max) ** 2, np.inf)
    M = ch[ks] - 0.5 * rho_bar[ks] * (np.sqrt(np.maximum(2.0 * (ch0[ks] - m0), 0.0)) + d[ks]) ** 2
    return U, M


def native(ref, cur, margin=0.0):
    """mimo_host_estep_certificate -> ((c^0, c^, rho, rho_bar, d), the four constants, the table of the certified pass)"""
    ref = [np.ascontiguousarray(x, dtype=float) for x in ref]
    cur = [np.ascontiguousarray(x, dtype=float) for x in cur]
    K, D = cur[1].shape
    out, table = np.full(5 * K + 4, np.nan), np.full(4 + 2 * K, np.nan)
    rc = _lib.load().mimo_host_estep_certificate(K, D, *[x.ctypes.data for x in ref + cur], float(margin), out.ctypes.data, table.ctypes.data)
    assert rc == 0, rc
    return tuple(out[i * K:(i + 1) * K] for i in range(5)), out[5 * K:], table


def bounds_built(cert, table):
    """(U_n, M_n) as the certified pass evaluates them: U_n = max_c (alpha_c + beta_c a0), M_n = gamma_k* + delta_k* m0"""
    ks, m0, a0 = cert
    K = (len(table) - 4) // 2
    U = np.maximum(table[0] + table[1] * a0, table[2] + table[3] * a0)
    return U, table[4:4 + K][ks] + table[4 + K:][ks] * m0


def one_group(prov, row_block, n_blocks=4):
    """share of (tile, wave) pairs that evaluate at most 16 rows: the tile's unproven rows and the proven ones of the wave's block"""
    n = len(prov) // T * T
    unproven = (~prov[:n]).reshape(-1, T).sum(axis=1)
    own = np.stack([(prov[:n] & (row_block[:n] == w)).reshape(-1, T).sum(axis=1) for w in range(n_blocks)], axis=1)
    return float(((unproven[:, None] + own) <= 16).mean())


# ---- (a) soundness ---------------------------------------------------------------------------------------------------------------
def _random_spd(rng, K, D, scale):
    A = rng.standard_normal((K, D, D))
    return scale * (np.einsum("kij,klj->kil", A, A) / D + 0.3 * np.eye(D))


def _canonical(mu, W, c_hat):
    b = np.einsum("kij,kj->ki", W, mu)
    return c_hat - 0.5 * np.einsum("kd,kd->k", b, mu), b, W


@pytest.mark.parametrize("D", [14, 16])
@pytest.mark.parametrize("move", [0.0, 1e-3, 0.03, 0.3, 3.0])
@pytest.mark.parametrize("seed", [0, 1])
def test_bounds_hold_on_every_row_and_component(D, move, seed):
    """U_n >= l_k(x_n) for every k outside the block and M_n <= max_k l_k(x_n) on every row, in both forms, for moves from nothing
    (0) over what one iteration does near convergence (1e-3, 0.03: means by that many sigma, precisions and peaks by that
    fraction) to moves that leave nothing provable (3).  Ten components sit 800 nats under the others, as the components
    without data do in a fit."""
    rng = np.random.default_rng(1000 * seed + 10 * D + int(1000 * move))
    K, N = 64, 3000
    centres = rng.normal(0.0, 6.0, size=(24, D))
    mu0 = centres[rng.integers(24, size=K)] + 0.5 * rng.standard_normal((K, D))
    W0 = _random_spd(rng, K, D, 1.0) * np.exp(rng.normal(0.0, 0.5, size=K))[:, None, None]
    ch0 = rng.normal(-20.0, 8.0, size=K)
    ch0[rng.permutation(K)[:10]] = -800.0
    X = mu0[rng.integers(K, size=N)] + rng.standard_normal((N, D)) * rng.choice([0.3, 1.0, 3.0], size=(N, 1))
    sig = 1.0 / np.sqrt(np.linalg.eigvalsh(W0)[:, -1])
    mu = mu0 + move * sig[:, None] * rng.standard_normal((K, D))
    P = _random_spd(rng, K, D, 1.0)
    W = W0 * (1.0 + move * rng.uniform(-0.3, 0.3, size=K))[:, None, None] + move * 0.2 * P * np.trace(W0, axis1=1, axis2=2)[:, None, None] / D
    ch = ch0 + move * 10.0 * rng.standard_normal(K)
    ref, cur = _canonical(mu0, W0, ch0), _canonical(mu, W, ch)
    blk = blocks_of(block_order(mu0, np.full(K, 500.0)))
    L0, L = _log_densities(X, *ref), _log_densities(X, *cur)
    cert = certificates(L0, blk)
    outside = np.where(blk[:, None] != blk[cert[0]][None, :], L, -np.inf).max(axis=0)
    top = L.max(axis=0)
    tol = 1e-9 * (1.0 + np.abs(L).max(axis=0))                     # (f64 rounding of sums of terms of that size)
    shares = []
    for U, M in (bounds_one_class(cert, constants(ref, cur)), bounds_built(cert, native(ref, cur)[2])):
        assert (U + tol >= outside).all()
        assert (M - tol <= top).all()
        p = U - M <= LN_TAU - EPS
        assert (outside[p] - top[p] < LN_TAU).all()                 # a proven row is dead outside its block by the kernel's own test
        shares.append(p.mean())
    print("D %d move %g: %.3f of the rows proven with one set of constants, %.3f as built" % (D, move, shares[0], shares[1]))
    if move <= 1e-3:
        assert shares[1] > 0.2                                      # (the small moves are not vacuous)
    if move >= 3.0:
        assert shares == [0.0, 0.0]


# ---- the native constants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,move", [(64, 16, 0.0), (64, 16, 0.01), (64, 14, 0.3), (17, 3, 0.05), (1, 1, 0.2), (40, 15, 2.0)])
def test_native_constants_against_numpy(K, D, move):
    rng = np.random.default_rng(K + D)
    mu0 = rng.normal(0.0, 6.0, size=(K, D))
    W0 = _random_spd(rng, K, D, 1.0)
    ch0 = rng.normal(-20.0, 8.0, size=K)
    mu = mu0 + move * rng.standard_normal((K, D))
    W = W0 * (1.0 + move * rng.uniform(-0.3, 0.3, size=K))[:, None, None] + move * 0.2 * _random_spd(rng, K, D, 1.0)
    ref, cur = _canonical(mu0, W0, ch0), _canonical(mu, W, ch0 + move * rng.standard_normal(K))
    (ch0_n, ch_n, rho_n, rhob_n, d_n), four, table = native(ref, cur, margin=-41.0)
    ch0_e, ch_e, rho_e, rhob_e, d_e = constants(ref, cur)
    assert np.allclose(ch0_n, ch0_e, rtol=1e-12, atol=1e-12) and np.allclose(ch_n, ch_e, rtol=1e-12, atol=1e-12)
    assert np.allclose(d_n, d_e, rtol=1e-12, atol=1e-12 * (1.0 + np.abs(mu0).max()))
    assert (rho_n <= rho_e * (1.0 + 1e-12)).all() and (rhob_n >= rhob_e * (1.0 - 1e-12)).all()
    assert (rho_n >= 0.0).all() and (rho_n >= 0.5 * np.minimum(rho_e, 1.0) - 0.1).all()       # an enclosure, and no wider than the grid
    assert np.array_equal(four, [ch0_n.min(), ch_n.max(), rho_n.min(), d_n.max()])
    if move == 0.0:
        assert (rho_n == 1.0).all() and (rhob_n == 1.0).all() and (d_n == 0.0).all()
    # the table: the affine bound of the row's own maximum lies under the exact one for any m0 (the other side: the soundness test)
    a0, m0 = rng.normal(-200.0, 150.0, size=500), rng.normal(-25.0, 5.0, size=500)
    ks = rng.integers(K, size=500)
    m0 = np.minimum(m0, ch0_n[ks])
    _, M_t = bounds_built((ks, m0, a0), table)
    M_exact = ch_n[ks] - 0.5 * rhob_n[ks] * (np.sqrt(2.0 * (ch0_n[ks] - m0)) + d_n[ks]) ** 2 - 41.0
    fin = np.isfinite(rhob_n[ks])
    assert (M_t[fin] <= M_exact[fin] + 1e-9 * (1.0 + np.abs(M_exact[fin]))).all() and (M_t[~fin] <= -1e299).all()


def test_native_rejections():
    lib = _lib.load()
    K, D = 8, 4
    rng = np.random.default_rng(0)
    c, b, W = _canonical(rng.standard_normal((K, D)), _random_spd(rng, K, D, 1.0), rng.standard_normal(K))
    c, b, W = [np.ascontiguousarray(x) for x in (c, b, W)]
    out, table = np.zeros(5 * K + 4), np.zeros(4 + 2 * K)
    p = [x.ctypes.data for x in (c, b, W, c, b, W)]

    def call(K_, D_, ptrs, o=out.ctypes.data, t=table.ctypes.data):
        return lib.mimo_host_estep_certificate(K_, D_, *ptrs, -41.0, o, t)

    assert call(K, D, p) == 0 and call(K, D, p, t=None) == 0
    assert call(0, D, p) == _lib.E_INVALID and call(K, 0, p) == _lib.E_INVALID and call(K, D, p, o=None) == _lib.E_INVALID
    for i in range(6):
        assert call(K, D, p[:i] + [None] + p[i + 1:]) == _lib.E_INVALID
    assert call(257, 1, p) == _lib.E_UNSUPPORTED and call(1, 33, p) == _lib.E_UNSUPPORTED
    for bad in (np.nan, np.inf):
        for arr, idx in ((c, 3), (b, (2, 1)), (W, (5, 1, 2))):
            keep = arr[idx]
            arr[idx] = bad
            assert call(K, D, p) == _lib.E_INVALID
            arr[idx] = keep
    W[2] = -W[2]                                                    # not positive definite
    assert call(K, D, p) == _lib.E_INVALID


def test_estep_certificate_under_asan_ubsan(tmp_path):
    """K = 1 .. 256, D = 1 .. 32 in a stand-alone program with its own main: nothing is loaded into this process."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "estep_certificate_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-mavx2", "-mfma", "-pthread", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # is the sanitizer runtime there?  An empty program decides that, so no error of the real build can hide as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([hipcc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    build = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tests", "estep_certificate_check.cpp"),
                                              os.path.join(ROOT, "mimo_amd", "csrc", "mimo_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "estep certificate ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]


# ---- (b) potential on the benchmark's fit -----------------------------------------------------------------------------------------
def run_policy(passes, built):
    """passes: per iteration (params, order, L).  The library's policy (cert_plan, mimo_abi.cpp): certificates in force whose
    partition is this pass's and that are under RENEW certified passes old -> certified; else a partition that has stood for two
    passes -> reference; else plain.  -> per iteration (kind, proven share, one-group share)."""
    state, prev_part, out = None, None, []
    for params, order, L in passes:
        blk, part = blocks_of(order), partition(order)
        stood, prev_part = part == prev_part, part
        if state is not None and state["part"] != part:
            state = None
        if state is not None and state["age"] < RENEW:
            cert = state["cert"]
            U, M = bounds_built(cert, native(state["ref"], params)[2]) if built else bounds_one_class(cert, constants(state["ref"], params))
            p = U - M <= LN_TAU - EPS
            outside = np.where(blk[:, None] != blk[cert[0]][None, :], L, -np.inf).max(axis=0)
            assert (outside[p] - L.max(axis=0)[p] < LN_TAU).all()    # what the kernel's own test finds on the proven rows
            state["age"] += 1
            out.append(("certified", float(p.mean()), one_group(p, blk[cert[0]])))
        elif stood:
            state = dict(ref=params, part=part, cert=certificates(L, blk), age=0)
            out.append(("reference", 0.0, 0.0))
        else:
            out.append(("plain", 0.0, 0.0))
    return out


def benchmark_passes(n_iter=25, N=24576):
    import bench
    from oracle_engine import OracleEngine
    from scipy.special import logsumexp
    from mimo_amd.distributions import native_sweep
    from mimo_amd.engine import SuffStats
    from mimo_amd.mixtures.gmm import _component_stats

    D, K = 16, 64
    X = bench.make_data(N, D, K, seed=1337, device="cpu").numpy()
    eng = OracleEngine()
    eng.upload(X)
    model = bench.build_model(bench.CONFIGS["c2"], eng)
    S = eng.label_stats(np.random.default_rng(4242).integers(0, K, size=N).astype(np.int32), K)
    passes = []
    for _ in range(n_iter):
        fused = native_sweep.gmm_vi_sweep(model.gating, model.components, _component_stats(S, model.components), S.gating_counts)
        assert fused is not None
        (c, b, W), bound = fused
        L = _log_densities(X, c, b, W)
        passes.append(((c.copy(), b.copy(), W.copy()), np.array(bound.block_order), L))
        S = SuffStats(*_packed_stats(X, np.exp(L - logsumexp(L, axis=0))))
    return passes


def test_model_of_the_benchmark_fit():
    """24 576 rows of bench.make_data (c2: D = 16, K = 64) from the benchmark's random hard-label start, 25 iterations of the
    public driver on the CPU oracle under mimo_host_block_order's order and the library's refresh policy.  The figure: the share
    of the wave-tiles of iterations 11 - 25 that run one column group (a reference or plain pass counts 0).

    One set of constants over all components: 0.000 — five components hold no data and sit at the prior's peak, c^ = -810 against
    -19 .. -10 of the others, so C0_min puts Q_n below zero for every row the other 59 components would prove (g ~ 390): no-go at
    the bar of one half.  As built (two classes, affine bounds, the native enclosure): the partition stands from iteration 8,
    iteration 9 is the reference pass, iterations 10 - 25 prove 0.98 - 0.99 of the rows and run 0.997 of the wave-tiles on one
    column group."""
    passes = benchmark_passes()
    figures = []
    for built in (False, True):
        out = run_policy(passes, built)
        for it, (kind, share, one) in enumerate(out, start=1):
            print("%s  iteration %2d  %-9s  proven %.4f   wave-tiles with <= 16 rows %.4f"
                  % ("as built " if built else "one class", it, kind, share, one))
        figures.append(float(np.mean([one for _, _, one in out[10:25]])))
        print("%s: wave-tiles of iterations 11 - 25 on one column group: %.4f" % ("as built" if built else "one class", figures[-1]))
        assert [kind for kind, _, _ in out].count("reference") >= 1
    assert figures[0] < 0.5 <= figures[1]
