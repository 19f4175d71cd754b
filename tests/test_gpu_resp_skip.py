"""Responsibility skip of the fused mean-field pass (mimo_tune "resp_skip_log2"): the statistics of a row block leave out
the rows whose weights there are all below tau = 2^-v.  Checked against the oracle, against the dense pass (v = 0) of the
same engine, for bit-identical repeats and for the error bound tau * sum_n |phi_nf| at weights just below / above tau."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

# all on the fused kernel (ROUTING.md).  The skip instantiations exist for Dz >= 14 (no occupancy cost there); (16, 50) has
# padding in its last row block.  Below Dz = 14 the key must leave the dense kernel in place: (8, 40) has 2 K16 < 8 slots
# per lane.
SKIP_SHAPES = [(16, 64), (16, 50), (14, 64)]
DENSE_SHAPES = [(12, 64), (8, 40)]
SHAPES = SKIP_SHAPES + DENSE_SHAPES


def _params(rng, D, K, spread):
    mus = rng.standard_normal((K, D)) * spread
    A = rng.standard_normal((K, D, D)) * 0.2
    W = A @ A.transpose(0, 2, 1) + np.eye(D)
    b = np.einsum("kij,kj->ki", W, mus)
    c = -0.5 * np.einsum("ki,ki->k", b, mus) + 0.5 * np.linalg.slogdet(W)[1] + rng.standard_normal(K) * 0.1
    return mus, c, b, W


def _data(rng, mus, N):
    return np.ascontiguousarray(mus[rng.integers(len(mus), size=N)] + rng.standard_normal((N, mus.shape[1])))


def _pass(engine, v, c, b, W):
    engine.tune("resp_skip_log2", v)
    S, sc = engine.estep(c, b, W)
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()]), sc.copy()


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("D,K", SHAPES)
@pytest.mark.parametrize("spread", [6.0, 0.3], ids=["separated", "overlapping"])
def test_skip_matches_oracle_and_dense(engine, D, K, spread):
    rng = np.random.default_rng(100 * D + K)
    mus, c, b, W = _params(rng, D, K, spread)
    Z = _data(rng, mus, 20000 + 13)          # ragged last tile
    engine.upload(Z)
    try:
        assert engine.plan(K)["kind"] == "fused"
        skip, sc_skip = _pass(engine, 60, c, b, W)
        skip2, sc_skip2 = _pass(engine, 60, c, b, W)
        dense, sc_dense = _pass(engine, 0, c, b, W)
        engine.tune("resp_skip_log2", 60)
        engine.estep_async(c, b, W)
        S_a, sc_a = engine.estep_wait()
    finally:
        engine.tune("resp_skip_log2", 60)
    L = O.canonical_eval(Z, c, b, W)
    lse = logsumexp(L, axis=0)
    n, sx, sxx = O.packed_stats(Z, np.exp(L - lse))
    ref = np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)])
    assert _rel(skip, ref) < 1e-11
    assert _rel(skip, dense) < 1e-13
    assert np.array_equal(sc_skip, sc_dense, equal_nan=True)            # the ELBO scalars come from the normalise phase alone
    assert abs(sc_skip[0] - lse.sum()) / abs(lse.sum()) < 1e-11
    assert np.array_equal(skip, skip2) and np.array_equal(sc_skip, sc_skip2, equal_nan=True)
    async_ = np.concatenate([S_a.n.ravel(), S_a.sx.ravel(), S_a.sxx.ravel()])
    assert np.array_equal(async_, skip) and np.array_equal(sc_a, sc_skip, equal_nan=True)


@pytest.mark.parametrize("D,K", DENSE_SHAPES)
def test_dense_kernel_below_dz14(engine, D, K):
    """No skip instantiation below Dz = 14: the statistics are the dense kernel's, bit for bit, whatever the key says."""
    rng = np.random.default_rng(7 * D + K)
    mus, c, b, W = _params(rng, D, K, 6.0)
    engine.upload(_data(rng, mus, 9000 + 7))
    try:
        assert engine.plan(K)["kind"] == "fused"
        skip, sc_skip = _pass(engine, 20, c, b, W)
        dense, sc_dense = _pass(engine, 0, c, b, W)
    finally:
        engine.tune("resp_skip_log2", 60)
    assert np.array_equal(skip, dense) and np.array_equal(sc_skip, sc_dense, equal_nan=True)


@pytest.mark.parametrize("D,K", SKIP_SHAPES)
@pytest.mark.parametrize("side", [-1, 1], ids=["below", "above"])
def test_skip_bound_at_threshold(engine, D, K, side):
    """Every datum has the same responsibilities (shared b, W): the unnormalised weights of the last row block sit just
    below or above tau = 2^-20.  Below: the block receives nothing (so the skip kernel ran), and each entry moves by at
    most tau * sum_n |phi_nf|.  Above: nothing is left out."""
    rng = np.random.default_rng(11)
    v = 20
    k0 = 16 * ((K - 1) // 16)
    Z = rng.standard_normal((5000 + 3, D))
    W = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    b = np.zeros((K, D))
    c = np.zeros(K)
    c[k0:] = -v * np.log(2.0) + side * 0.01    # l - max l = c_k: e of the last block is tau * e^(+-0.01)
    engine.upload(Z)
    try:
        assert engine.plan(K)["kind"] == "fused"
        skip, sc_skip = _pass(engine, v, c, b, W)
        dense, sc_dense = _pass(engine, 0, c, b, W)
    finally:
        engine.tune("resp_skip_log2", 60)
    assert np.array_equal(sc_skip, sc_dense, equal_nan=True)
    N = len(Z)
    Zt = np.hstack([Z, np.ones((N, 1))])
    absphi = np.abs(Zt).T @ np.abs(Zt)                     # sum_n |z~_a z~_b|
    bound_n = np.full(K, float(N))
    bound_sx = np.tile(absphi[D, :D], (K, 1))
    bound_sxx = np.tile(absphi[:D, :D], (K, 1, 1))
    bound = np.concatenate([bound_n, bound_sx.ravel(), bound_sxx.ravel()]) * 2.0 ** -v
    diff = np.abs(skip - dense)
    assert np.all(diff <= bound + 1e-13 * np.max(np.abs(dense)))
    n_skip = skip[:K]
    if side < 0:
        assert np.all(n_skip[k0:] == 0.0) and np.all(dense[k0:K] > 0.0) and np.all(n_skip[:k0] > 0.0)
    else:
        assert _rel(skip, dense) < 1e-13
