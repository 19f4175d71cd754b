"""The per-datum reductions of the normalise phase with their lane exchanges in registers (DPP row rotate for lane ^ 8,
v_permlane16_swap / v_permlane32_swap for lane ^ 16 / ^ 32; mimo_device.h: lane_xor_max, lane_xor_sum) instead of
__shfl_xor: same stages, same order, bit for bit the same sums and maxima (profiles/r08_c2_lane_exchange.txt).

  self-test     one wave runs every helper next to the __shfl_xor form of the same stage (mimo_lane_exchange_selftest): the
                only place where the half-exchange semantics of the two swaps are checked in isolation.
  softmax       passes through the public engine against the oracle at the tolerances of tests/test_gpu_fused_valu.py
                (statistics 1e-11, sum of the log-normalisers and the lse table 1e-12, 1e-11 for the skip family, whose key-60
                pass also stays within 1e-13 of its key-0 pass with bit-equal scalars).  N = 33 and 97: two and four tiles of
                32 rows with a ragged last one, so lanes of rows past N sit in every exchange beside live ones.
  repeats       the same pass twice, and the synchronous against the asynchronous call: bit-identical.
  generic       a pass with one NaN row and one with row weights: the sum_k e l tree runs in the generic kernel only.

A wrong exchange pairs a lane with the wrong partner: the maximum or the sum of a datum then misses some of its eight
parts, and the weights of that row do not sum to one — far outside every tolerance here, at any N."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

NS = [33, 97]


def _params(rng, D, K, spread):
    """As tests/test_gpu_fused_valu.py: centres ~ N(0, spread^2 I), precisions near I."""
    mus = rng.standard_normal((K, D)) * spread
    A = rng.standard_normal((K, D, D)) * 0.2
    W = A @ A.transpose(0, 2, 1) + np.eye(D)
    b = np.einsum("kij,kj->ki", W, mus)
    c = -0.5 * np.einsum("ki,ki->k", b, mus) + 0.5 * np.linalg.slogdet(W)[1] + rng.standard_normal(K) * 0.1
    return mus, c, b, W


def _data(rng, mus, N):
    return np.ascontiguousarray(mus[rng.integers(len(mus), size=N)] + rng.standard_normal((N, mus.shape[1])))


def _vec(S):
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()])


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


_CASES = {}


def _case(D, K, N):
    """Problem and oracle result of a shape, computed once and shared (read-only) by the tests that use it."""
    key = (D, K, N)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * K + N)
        mus, c, b, W = _params(rng, D, K, 2.0)
        Z = _data(rng, mus, N)
        L = O.canonical_eval(Z, c, b, W)
        lse = logsumexp(L, axis=0)
        n, sx, sxx = O.packed_stats(Z, np.exp(L - lse))
        ref = np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)])
        for arr in (Z, c, b, W, L, lse, ref):
            arr.setflags(write=False)
        _CASES[key] = (Z, c, b, W, L, lse, ref)
    return _CASES[key]


def _plain(engine, key, c, b, W):
    engine.tune("resp_skip_log2", key)
    S, sc = engine.estep(c, b, W)
    return _vec(S), sc.copy()


def _check_plain(engine, c, b, W, lse, ref, skip_family):
    """Plain pass against the oracle; skip family: resp_skip_log2 = 60 and 0.  Twice, and asynchronously: the same bits."""
    try:
        got, sc = _plain(engine, 60, c, b, W)
        again, sc_again = _plain(engine, 60, c, b, W)
        engine.estep_async(c, b, W)
        S_a, sc_a = engine.estep_wait()
        if skip_family:
            dense, sc_dense = _plain(engine, 0, c, b, W)
    finally:
        engine.tune("resp_skip_log2", 60)
    assert _rel(got, ref) < 1e-11
    assert abs(sc[0] - lse.sum()) <= (1e-11 if skip_family else 1e-12) * abs(lse.sum())
    assert np.array_equal(again, got) and np.array_equal(sc_again, sc, equal_nan=True)
    assert np.array_equal(_vec(S_a), got) and np.array_equal(sc_a, sc, equal_nan=True)
    if skip_family:
        assert _rel(dense, ref) < 1e-11
        assert _rel(got, dense) < 1e-13
        assert np.array_equal(sc, sc_dense, equal_nan=True)


def _check_generic(engine, c, b, W, lse, ref):
    """The same pass with the lse table kept: the generic instantiation of the tile kernels (sum_k e l tree included)."""
    S, sc = engine.estep(c, b, W, keep_lse=True)
    assert _rel(_vec(S), ref) < 1e-11
    assert abs(sc[0] - lse.sum()) <= 1e-12 * abs(lse.sum())
    assert _rel(engine.get_lse(), lse) < 1e-12
    S2, sc2 = engine.estep(c, b, W, keep_lse=True)
    assert np.array_equal(_vec(S2), _vec(S)) and np.array_equal(sc2, sc, equal_nan=True)


def test_selftest(engine):
    assert engine.lane_exchange_selftest() == 0


# (Dz, K, kind of the plain pass, skip family, mid kernels moved out of the way).  Beside each row: the instantiations it runs
# (plain pass; generic request), all of which take the register form — a row whose instantiation is put on a kernel's keep-list
# (fused_lane_regs, mid_lane_regs, vi_rowwave_lane_regs, small_lane_regs) no longer tests it and needs another shape.
SOFTMAX_SHAPES = [
    (16, 64, "fused", True, False),          # fused_kernel<10,1,kFastVI,16,0,true> and <..,false> (keys 60, 0), FULL path; <10,1,kGeneric,16>
    (12, 64, "fused", False, False),         # fused_kernel<6,1,kFastVI,12>, three workgroups per CU; <6,1,kGeneric,12>
    (16, 48, "fused", True, True),           # the Dz = 16 kernels again, K16 = 3: 6 slots per lane, no padding components
    (16, 40, "fused", True, True),           # ... K16 = 3 with 8 padding components
    (5, 32, None, False, False),             # fused_kernel<2,1,kGeneric,5>, K16 = 2: 4 slots per lane (the plain pass is the narrow kernels')
    (8, 256, None, False, False),            # fused_kernel<3,4,kFastVI,8> and <3,4,kGeneric,8>: the chunked normalisation
    (20, 80, "mid", False, False),           # mid_kernel<20,5,4,0>
    (2, 16, "small", False, False),          # small_kernel<2,4,4,kFastVI / kGeneric>: 4 lanes per row (masks 1, 2)
    (4, 8, "small", False, False),           # small_kernel<4,2,4,..>: two components per lane
    (8, 32, "rowwave-vi", False, False),     # vi_rowwave_kernel<2,3> (K = 64 at this Dz would be <4,3>, which keeps __shfl_xor)
]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D,K,kind,skip,no_mid", SOFTMAX_SHAPES)
def test_softmax_against_oracle(engine, D, K, kind, skip, no_mid, N):
    Z, c, b, W, _, lse, ref = _case(D, K, N)
    engine.upload(Z)
    try:
        if no_mid:
            engine.tune("mid_min_d", 64)         # K = 40, 48 at Dz = 16 would otherwise take the mid kernel (ROUTING.md)
        if kind is not None:
            assert engine.plan(K)["kind"] == kind
        _check_plain(engine, c, b, W, lse, ref, skip_family=skip)
        _check_generic(engine, c, b, W, lse, ref)
    finally:
        engine.tune("mid_min_d", 0)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D,K,kind,keep_logp", [
    (8, 64, None, True),                         # fused_kernel<3,1,kGeneric,8> in label mode (the table takes it off the row-owner kernels)
    (8, 256, None, True),                        # fused_kernel<3,4,kGeneric,8>: chunked
    (5, 100, "rowwave", False),                  # gibbs_rowwave_kernel<8,2>
    (24, 160, "rowwave", False),                 # gibbs_stream_kernel<10,..> (every instantiation takes the register form)
    (20, 16, "mid", False),                      # mid_kernel<20,1,..,1>: label mode (every instantiation takes the register form)
    (4, 8, "small", False),                      # small_kernel<4,2,4,kFastGibbs>
])
def test_label_counts_against_oracle(engine, D, K, kind, keep_logp, N):
    """The count trees of the label draw: labels exact against the oracle with host uniforms, twice the same."""
    Z, c, b, W, L, _, _ = _case(D, K, N)
    u = np.random.default_rng(7 * D + K + N).random(N)
    ref = O.sample_discrete_from_log(L, u)
    engine.upload(Z)
    if kind is not None:
        assert engine.plan(K, gibbs=True)["kind"] == kind
    lab, S = engine.gibbs_labels(c, b, W, u=u, keep_logp=keep_logp)
    assert np.array_equal(lab, ref)
    assert np.array_equal(S.n, np.bincount(ref, minlength=K))
    lab2, S2 = engine.gibbs_labels(c, b, W, u=u, keep_logp=keep_logp)
    assert np.array_equal(lab2, lab) and np.array_equal(_vec(S2), _vec(S))
    if keep_logp:
        assert _rel(engine.get_logp(), L) < 1e-12


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D,K", [(16, 64), (16, 40), (8, 256)])
def test_generic_kernel_nan_row_and_row_weights(engine, D, K, N):
    """One row with a NaN (zeroed, its weight 0 in the statistics, its lse at z = 0 in the bound) and a pass with row weights:
    both run the generic kernel, the only one with the sum_k e l tree (entropy split of the bound: scalars[1], [2])."""
    Z, c, b, W, L, lse, _ = _case(D, K, N)
    R = np.exp(L - lse)
    engine.upload(Z)
    w = np.random.default_rng(D + K + N).uniform(0.0, 2.0, size=N)
    n, sx, sxx = O.packed_stats(Z, R * w[None, :])
    S, sc = engine.estep(c, b, W, row_weights=w, entropy_split=True)
    assert _rel(S.n, n) < 1e-11 and _rel(S.sx, sx) < 1e-11 and _rel(S.sxx, sxx) < 1e-11
    assert abs(sc[0] - lse.sum()) <= 1e-12 * abs(lse.sum())
    srl = float(np.sum(np.where(R > 0, R * L, 0.0)))
    assert abs(sc[1] - srl) <= 1e-11 * abs(srl)
    S2, sc2 = engine.estep(c, b, W, row_weights=w, entropy_split=True)
    assert np.array_equal(_vec(S2), _vec(S)) and np.array_equal(sc2, sc, equal_nan=True)

    bad = N // 2
    Zn = Z.copy(); Zn[bad, D - 1] = np.nan
    Zc = Z.copy(); Zc[bad] = 0.0
    mask = np.ones(N); mask[bad] = 0.0
    Lc = O.canonical_eval(Zc, c, b, W)
    lsec = logsumexp(Lc, axis=0)
    n, sx, sxx = O.packed_stats(Zc, np.exp(Lc - lsec) * mask[None, :])
    try:
        engine.upload(Zn)
        assert engine.n_bad == 1
        S, sc = engine.estep(c, b, W)
        assert _rel(S.n, n) < 1e-11 and _rel(S.sx, sx) < 1e-11 and _rel(S.sxx, sxx) < 1e-11
        assert abs(sc[0] - lsec.sum()) <= 1e-12 * abs(lsec.sum())
    finally:
        engine.upload(Z)
    assert engine.n_bad == 0
