"""The fused fast VI kernels whose feature count is 1 mod 4 (Dz = 13 and 16, one row block per wave, dense and skipping) start
the accumulators of L = Theta . Phi' at the constant c_k and leave out the contraction step that held nothing but the constant
feature (mimo_kernels.hip, SEED).  What can go wrong: a lane seeds the wrong component, the Theta ring (one step shorter, two
dummy refills at Dz = 16) loses its place from tile to tile, a row past N (l = c_k now, not 0) leaks into a sum, a large or
switched-off constant meets a path that expected the accumulators to start at zero.

Shapes: (Dz 16, K 64) every lane owns 8 slots; (Dz 16, K 40) three row blocks, padding components in the last, one wave without a
block; (Dz 13, K 64) the dense kernel alone; (Dz 15, K 64) the control, whose kernels do not change.  N = 31 and 33 are one tile
and two tiles with rows past N; at N = 4099 the grid is cut to two workgroups (mimo_tune "num_cu" = 1), so each walks 64 or 65
tiles and the ring wraps that often.  Tolerances are those of tests/test_gpu_parity.py for the fast pass at these shapes
(test_many_tiles_per_workgroup): statistics 1e-11 of the largest entry, the sum of the log-normalisers 1e-12 relative."""
import numpy as np
import pytest
from scipy.special import digamma, logsumexp

from conftest import rel_err
from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64), (16, 40), (13, 64), (15, 64)]
ROWS = [31, 33, 4099]


def _problem(D, K, N):
    """W = I, means 40 apart; every third component shares its mean (up to 0.3) with the one 16 further on, so that a good part
    of the rows split their weight between two row blocks; rows drawn around the means of all components."""
    rng = np.random.default_rng(1500 + 100 * D + K + N)
    k = np.arange(K)
    mus = np.zeros((K, D))
    mus[k, k % D] = 40.0 * (1 + k // D)
    pairs = [(a, a + 16) for a in range(0, K - 16, 3)]
    for a, a2 in pairs:
        mus[a2] = mus[a] + 0.3 * rng.standard_normal(D)
    W = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    b = mus.copy()
    c = -0.5 * np.einsum("ki,ki->k", b, mus) + rng.standard_normal(K) * 0.1
    Z = np.ascontiguousarray(mus[rng.integers(K, size=N)] + rng.standard_normal((N, D)))
    return Z, c, b, W, pairs


def _oracle(Z, c, b, W, drop=()):
    """statistics (rows `drop` left out of them) and the sum of the log-normalisers over all rows"""
    L = O.canonical_eval(Z, c, b, W)
    lse = logsumexp(L, axis=0)
    R = np.exp(L - lse)
    R[:, list(drop)] = 0.0
    n, sx, sxx = O.packed_stats(Z, R)
    return np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)]), float(lse.sum())


_REF = {}


def _reference(D, K, N):
    if (D, K, N) not in _REF:
        Z, c, b, W, _ = _problem(D, K, N)
        _REF[(D, K, N)] = _oracle(Z, c, b, W)
    return _REF[(D, K, N)]


def _flat(S):
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()])


def _pass(engine, key, c, b, W):
    engine.tune("resp_skip_log2", key)
    S, sc = engine.estep(c, b, W)
    return _flat(S), sc.copy()


@pytest.fixture(scope="module")
def fresh():
    from mimo_amd.engine import HipEngine
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.fixture
def fused_engine(engine):
    engine.tune("mid_min_d", 64)                                   # K <= 48 at these Dz would otherwise take the mid kernel (ROUTING.md)
    yield engine
    engine.tune("resp_skip_log2", 60)
    engine.tune("mid_min_d", 0)
    engine.tune("num_cu", 0)


def _upload(engine, Z, K):
    engine.upload(Z)
    if len(Z) > 1000:
        engine.tune("num_cu", 1)                                   # two workgroups: dozens of tiles each
    assert engine.plan(K)["kind"] == "fused"


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("D,K", SHAPES)
def test_pass_against_the_oracle(fused_engine, fresh, D, K, N):
    """Skipping (key 60) and dense (key 0) pass against the oracle, bit-equal scalars between the two; a repeat, the asynchronous
    call and a fresh context return the same bits."""
    engine = fused_engine
    Z, c, b, W, _ = _problem(D, K, N)
    ref, ref_lse = _reference(D, K, N)
    _upload(engine, Z, K)
    if N > 1000:
        assert engine.plan(K)["workgroups"] * 16 <= (N + 31) // 32     # every workgroup walks dozens of tiles
    skip, sc_skip = _pass(engine, 60, c, b, W)
    dense, sc_dense = _pass(engine, 0, c, b, W)
    skip2, sc_skip2 = _pass(engine, 60, c, b, W)
    engine.estep_async(c, b, W)
    S_a, sc_a = engine.estep_wait()
    print("Dz=%d K=%d N=%d: skip vs oracle %.2e, dense vs oracle %.2e, lse %.2e"
          % (D, K, N, rel_err(skip, ref), rel_err(dense, ref), abs(sc_skip[0] - ref_lse) / abs(ref_lse)))
    assert rel_err(skip, ref) < 1e-11 and rel_err(dense, ref) < 1e-11
    assert abs(sc_skip[0] - ref_lse) < 1e-12 * abs(ref_lse)
    assert np.array_equal(sc_skip, sc_dense, equal_nan=True)
    assert np.array_equal(skip, skip2) and np.array_equal(sc_skip, sc_skip2, equal_nan=True)
    assert np.array_equal(_flat(S_a), skip) and np.array_equal(sc_a, sc_skip, equal_nan=True)
    try:
        _upload(fresh, Z, K)                                       # (the same grid: the partial blocks are summed in launch order)
        for key, want in ((60, (skip, sc_skip)), (0, (dense, sc_dense))):
            got = _pass(fresh, key, c, b, W)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    finally:
        fresh.tune("resp_skip_log2", 60)
        fresh.tune("num_cu", 0)


@pytest.mark.parametrize("shift", [0.0, 2.0e4], ids=["negative", "positive"])
@pytest.mark.parametrize("D,K", SHAPES)
def test_large_constants_a_switched_off_component_and_a_nan_row(fused_engine, D, K, shift):
    """c_k = (quadratic part) + E[log pi_k] of gating counts scaled down to 1e-4 .. 4e-4: digamma(alpha) ~ -1 / alpha puts the
    constants at -1e4 .. -2.5e3, thousands apart, against rows a few units from their means (with the shift: +1e4 .. +1.75e4, the
    other sign).  The two components of an overlapping pair share their count, so their rows still split their weight.  One
    component that owns rows is switched off (c = -inf).  Once on finite data (the fast kernel), once with a NaN in one row:
    that row carries l = c_k, counts in the sum of the log-normalisers and stays out of the statistics.  In both, sum_k n_k is the
    number of finite rows."""
    engine = fused_engine
    N = 4099
    Z, c, b, W, pairs = _problem(D, K, N)
    rng = np.random.default_rng(77 + D + K)
    alpha = 1e-4 * (1.0 + 3.0 * rng.random(K))
    for a, a2 in pairs:
        alpha[a2] = alpha[a]
    c = c + digamma(alpha) - digamma(alpha.sum()) + shift
    assert 2e3 < np.abs(c).max() < 4e4 and np.ptp(c) > 5e3
    off = 20                                                       # no partner in a pair; second row block
    assert all(off not in p for p in pairs)
    c[off] = -np.inf
    bad = 2 * 32 + 9                                               # third tile, second wave
    Zn = Z.copy()
    Zn[bad, D // 2] = np.nan
    Z0 = Zn.copy()
    Z0[bad] = 0.0                                                  # what the pass computes on: l = c_k for that row
    for data, zref, drop in ((Z, Z, ()), (Zn, Z0, (bad,))):
        ref, ref_lse = _oracle(zref, c, b, W, drop)
        _upload(engine, data, K)
        assert engine.n_bad == len(drop)
        for key in (60, 0):
            got, sc = _pass(engine, key, c, b, W)
            n_sum = got[:K].sum()
            print("Dz=%d K=%d shift=%g nan=%d key=%d: vs oracle %.2e, lse %.2e, sum n - rows %.2e"
                  % (D, K, shift, len(drop), key, rel_err(got, ref), abs(sc[0] - ref_lse) / abs(ref_lse), n_sum - (N - len(drop))))
            assert rel_err(got, ref) < 1e-11
            assert abs(sc[0] - ref_lse) < 1e-12 * abs(ref_lse)
            assert abs(n_sum - (N - len(drop))) <= 1e-12 * (N - len(drop))
            assert got[off] < 1e-290 and np.all(np.isfinite(got))
