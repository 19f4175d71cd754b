"""The three places where the fused tile kernel's per-tile VALU work was trimmed, at the shapes where each can go wrong
(every form computes bit for bit what the one before it did, so these pin results, not speed: profiles/r07_c2_valu_trim.txt):

  feature build   the parity of a feature pair rides on an LDS address (a second read of the z~ row, one element further on in
                  the upper half of the wave); only the pairs that straddle the end of a triangle row keep a select.  Odd and
                  even Dz put the straddles at different parities, Dz = 1 and 2 are almost nothing but straddles and padding.
  live mask       K16 = 4: from the lane's own maximum, one ballot for all four row blocks; K16 < 4: per slot, as before.
  Z staging       the tile's place in Z is carried on the scalar side, a lane compares its element index with the number of
                  elements the tile has in Z: partial tiles, single tiles, tiles behind a workgroup's last one.

Each case is one pass through the public engine against the oracle at the tolerances of the parity tests of its family
(test_gpu_parity.py: statistics 1e-11, sum of the log-normalisers and the lse table 1e-12; test_gpu_resp_skip.py for the skip
kernels: 1e-11, and the key-60 pass within 1e-13 of the key-0 pass, the bound DESIGN.md section 4 states for the skip at this
key, with bit-equal scalars).  A plain request goes to the fused kernel only where the router sends the shape there (asserted);
a request that keeps the lse table always runs the generic instantiation of the fused kernel for K <= 64, Dz <= 16
(mimo_route.h: tables are not a plain request).

Which kernels carry the new forms: the fast VI instantiations with one row block per wave, not split, Dz >= 10 (feature build
and staging; the live mask in the three skip kernels at Dz >= 14) — the plain passes of Dz = 12 .. 16 below.  The generic,
split and label-mode instantiations keep the forms they had, because the new ones cost them registers; their
cases here (Dz = 1, 2, 7, the split shapes, the label pass, every generic request) hold the same feature map and the same
staging to the same oracle, so a later change that extends the new forms to them is already covered."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

T = 32
LN_TAU = -60 * np.log(2.0)


def _params(rng, D, K, spread):
    """As test_gpu_resp_skip._params: centres ~ N(0, spread^2 I), precisions near I."""
    mus = rng.standard_normal((K, D)) * spread
    A = rng.standard_normal((K, D, D)) * 0.2
    W = A @ A.transpose(0, 2, 1) + np.eye(D)
    b = np.einsum("kij,kj->ki", W, mus)
    c = -0.5 * np.einsum("ki,ki->k", b, mus) + 0.5 * np.linalg.slogdet(W)[1] + rng.standard_normal(K) * 0.1
    return mus, c, b, W


def _data(rng, mus, N):
    return np.ascontiguousarray(mus[rng.integers(len(mus), size=N)] + rng.standard_normal((N, mus.shape[1])))


def _oracle(Z, c, b, W):
    L = O.canonical_eval(Z, c, b, W)
    lse = logsumexp(L, axis=0)
    n, sx, sxx = O.packed_stats(Z, np.exp(L - lse))
    return L, lse, np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)])


def _vec(S):
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()])


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _plain(engine, key, c, b, W):
    engine.tune("resp_skip_log2", key)
    S, sc = engine.estep(c, b, W)
    return _vec(S), sc.copy()


def _check_plain(engine, c, b, W, lse, ref, skip_family):
    """Plain pass (fast VI kernel) against the oracle; skip family: key 60 against key 0 as well.  Returns the key-60 result."""
    try:
        got, sc = _plain(engine, 60, c, b, W)
        if skip_family:
            dense, sc_dense = _plain(engine, 0, c, b, W)
    finally:
        engine.tune("resp_skip_log2", 60)
    assert _rel(got, ref) < 1e-11
    assert abs(sc[0] - lse.sum()) <= (1e-11 if skip_family else 1e-12) * abs(lse.sum())
    if skip_family:
        assert _rel(dense, ref) < 1e-11
        assert _rel(got, dense) < 1e-13
        assert np.array_equal(sc, sc_dense, equal_nan=True)
    return got, sc


def _check_generic(engine, c, b, W, lse, ref):
    """The same pass with the lse table kept: generic instantiation of the fused kernel."""
    S, sc = engine.estep(c, b, W, keep_lse=True)
    assert _rel(_vec(S), ref) < 1e-11
    assert abs(sc[0] - lse.sum()) <= 1e-12 * abs(lse.sum())
    assert _rel(engine.get_lse(), lse) < 1e-12


# ---- feature map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [1, 2, 7, 12, 13, 14, 15, 16])
def test_feature_map(engine, D):
    """K = 64, N = 4099: every statistic is a sum over one feature, so a product built from the wrong pair of z~ entries
    shows in its column.  Dz = 12 is the dense kernel at three workgroups per CU, Dz = 14 .. 16 are the skip kernels; below
    Dz = 10 the plain pass belongs to other kernel families and only the generic request reaches the fused kernel."""
    K, N = 64, 4099
    rng = np.random.default_rng(500 + D)
    mus, c, b, W = _params(rng, D, K, 2.0)
    Z = _data(rng, mus, N)
    _, lse, ref = _oracle(Z, c, b, W)
    engine.upload(Z)
    if D >= 10:
        assert engine.plan(K)["kind"] == "fused"
        _check_plain(engine, c, b, W, lse, ref, skip_family=D >= 14)
    _check_generic(engine, c, b, W, lse, ref)


@pytest.mark.parametrize("K", [16, 32])
def test_split_path(engine, K):
    """Dz = 16, K <= 32: the split instantiations (one / two row blocks shared by the four waves) build the same feature tile
    from other waves' points of view.  K = 32 takes the fast VI one once the mid kernel is moved out of the way; the plain
    pass of K = 16 belongs to the narrow kernels, so that shape runs the generic request alone."""
    D, N = 16, 4099
    rng = np.random.default_rng(600 + K)
    mus, c, b, W = _params(rng, D, K, 2.0)
    Z = _data(rng, mus, N)
    _, lse, ref = _oracle(Z, c, b, W)
    engine.upload(Z)
    try:
        engine.tune("mid_min_d", 64)
        if K == 32:
            assert engine.plan(K)["kind"] == "fused"
            _check_plain(engine, c, b, W, lse, ref, skip_family=False)
        _check_generic(engine, c, b, W, lse, ref)
    finally:
        engine.tune("mid_min_d", 0)


def test_gibbs_path(engine):
    """One label pass at Dz = 8, K = 64 with host uniforms: labels exact, counts exact, statistics to 1e-11.  The logp table is
    kept, which takes the pass off the row-owner label kernels (a plain label pass at this shape is theirs) and onto the fused
    kernel in label mode: same feature map, same staging, the inverse-CDF draw instead of the softmax."""
    D, K, N = 8, 64, 4099
    rng = np.random.default_rng(700 + D)
    mus, c, b, W = _params(rng, D, K, 2.0)
    Z = _data(rng, mus, N)
    u = rng.random(N)
    L = O.canonical_eval(Z, c, b, W)
    ref = O.sample_discrete_from_log(L, u)
    n, sx, sxx = O.packed_stats(Z, O.one_hot(ref, K))
    engine.upload(Z)
    lab, S = engine.gibbs_labels(c, b, W, u=u, keep_logp=True)
    assert np.array_equal(lab, ref)
    assert np.array_equal(S.n, n) and _rel(S.sx, sx) < 1e-11 and _rel(S.sxx, sxx) < 1e-11
    assert _rel(engine.get_logp(), L) < 1e-12


# ---- live mask ----------------------------------------------------------------------------------------------------------------

def _planted_row(mus, home, k):
    """A point on the segment from centre `home` to centre `k` (W = I) where l_k - l_home = -1: component k carries a weight
    of e^-1 / (1 + e^-1) there, far above tau."""
    d = mus[k] - mus[home]
    t = 0.5 * (1.0 - 2.0 / (d @ d))
    return mus[home] + t * d


@pytest.mark.parametrize("K", [64, 40])
@pytest.mark.parametrize("scale", [1.0, 0.05], ids=["separated", "overlapping"])
def test_live_mask(engine, K, scale):
    """Dz = 16, key 60.  K = 64: a lane's 8 slots lie in one row block and the mask comes from the lane's maximum; K = 40
    (K16 = 3): 6 slots per lane, lane 2 (components 12 .. 17) straddles row blocks 0 and 1, per slot.  Separated clusters
    (centres ~ N(0, 6^2 I), W = I): nearly every row is live in its own row block alone.  Two rows are planted between their
    home centre and a centre of another row block, so that this component is the ONLY live one of that block for the row
    and holds a weight of 0.27: once the first slot of a lane, once the last — a mask that missed either would lose 0.27 of a
    count.  The design is checked with the oracle before the GPU is asked.  Overlapping clusters (centres x 0.05): every
    mask is full."""
    D, N = 16, 20 * T + 5
    cpp = 2 * ((K + 15) // 16)                              # slots per lane
    k_first, k_last, home = (24, 47, 60) if K == 64 else (12, 17, 39)
    assert k_first % cpp == 0 and k_last % cpp == cpp - 1 and len({k_first // 16, k_last // 16, home // 16}) == 3
    rng = np.random.default_rng(800 + K)
    mus = rng.standard_normal((K, D)) * 6.0 * scale
    W = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    b = mus.copy()
    c = -0.5 * np.einsum("ki,ki->k", mus, mus)
    Z = _data(rng, mus, N)
    rows = {3: k_first, 2 * T + 8: k_last}                   # two tiles, two waves
    if scale == 1.0:
        for r, k in rows.items():
            Z[r] = _planted_row(mus, home, k)
    L, lse, ref = _oracle(Z, c, b, W)
    hit = L - L.max(axis=0) >= LN_TAU                        # (K, N)
    blocks = np.add.reduceat(hit, np.arange(0, K, 16), axis=0) > 0
    if scale == 1.0:
        for r, k in rows.items():
            blk = slice(16 * (k // 16), 16 * (k // 16) + 16)
            assert list(np.flatnonzero(hit[blk, r]) + blk.start) == [k]
            assert abs(L[k, r] - L[home, r] + 1.0) < 1e-9 and np.argmax(L[:, r]) == home
        assert blocks.mean() < 0.5                           # most (row, block) pairs are dead
    else:
        assert blocks.all()
    engine.upload(Z)
    try:
        engine.tune("mid_min_d", 64)                         # K = 40 would otherwise take the mid kernel (ROUTING.md)
        assert engine.plan(K)["kind"] == "fused"
        _check_plain(engine, c, b, W, lse, ref, skip_family=True)
    finally:
        engine.tune("mid_min_d", 0)


# ---- Z staging ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [16, 15])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 32 * 5 + 7, 40000 + 13])
def test_z_staging(engine, D, N):
    """Single and partial tiles, and 1251 tiles over two workgroups per CU (a workgroup walks 2 or 3 tiles, one of them ends
    on the partial tile, and every workgroup prefetches one or two tiles that lie past the data).  At Dz = 15 a tile has
    480 elements, no multiple of the workgroup's 256 threads.  Plain pass (skip kernel, key 60 and key 0) and generic
    request; a repeat of the last plain call returns the same bits."""
    K = 64
    rng = np.random.default_rng(900 + 17 * D + N % 1000)
    mus, c, b, W = _params(rng, D, K, 3.0)
    Z = _data(rng, mus, N)
    _, lse, ref = _oracle(Z, c, b, W)
    engine.upload(Z)
    assert engine.plan(K)["kind"] == "fused"
    got, sc = _check_plain(engine, c, b, W, lse, ref, skip_family=True)
    again, sc_again = _plain(engine, 60, c, b, W)
    assert np.array_equal(again, got) and np.array_equal(sc_again, sc, equal_nan=True)
    _check_generic(engine, c, b, W, lse, ref)
