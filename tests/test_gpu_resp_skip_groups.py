"""Group structure of the fused mean-field pass's responsibility skip: the statistics of a row block contract its live
rows four at a time, the next group's operands refilled while the current group issues.  The data are built so that the
number of live rows per (tile, row block) is known: 0 (empty mask), 1 and 3 (one partial group), 4 (one full group), 5
and 29 (full groups and a remainder), 8 and 32 (full groups only, 32: all eight), plus every row live in every block,
ragged row counts and many tiles per workgroup.  The designed counts are checked with the oracle on the CPU before the
GPU result is looked at.

What these tests do and do not show: they pin the loop's results at every group count, so a change of its schedule that
drops, repeats or reorders a group fails here.  The pipelined loop computes bit for bit what the unpipelined one did, so
they cannot tell the two apart and say nothing about speed (profiles/r06_c2_skip_refill.txt does).  mimo_plan reports the
kernel family ("fused") but not whether the launch is the skip or the dense instantiation, and the two may differ by up
to 1e-13 only: a key of 60 that silently launched the dense kernel would pass."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

T = 32                                     # rows per tile
LN_TAU = -60 * np.log(2.0)                 # resp_skip_log2 = 60
BLOCK0_COUNTS = [0, 1, 3, 4, 5, 8, 29, 32]  # live rows of row block 0, tile by tile
# (15, 33): three row blocks, so one of the four waves owns none; (16, 50): padding in the last row block
SHAPES = [(16, 64), (16, 50), (14, 64), (15, 33)]


def _params(rng, D, K, scale):
    """W = I, means 40 apart (times scale), c as in test_gpu_resp_skip._params."""
    k = np.arange(K)
    mus = np.zeros((K, D))
    mus[k, k % D] = 40.0 * (1 + k // D) * scale
    W = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    b = mus.copy()
    c = -0.5 * np.einsum("ki,ki->k", b, mus) + rng.standard_normal(K) * 0.1
    return mus, c, b, W


def _components(rng, K, reps=1):
    """Component of every row, tile by tile: tile t has BLOCK0_COUNTS[t % 8] rows from row block 0, the others spread
    over the remaining row blocks, in random positions of the tile."""
    comps = []
    for t in range(reps * len(BLOCK0_COUNTS)):
        m = BLOCK0_COUNTS[t % len(BLOCK0_COUNTS)]
        own = rng.integers(0, 16, size=m)
        rest = 16 + (t + np.arange(T - m)) % (K - 16)
        comps.append(rng.permutation(np.concatenate([own, rest])))
    return np.concatenate(comps)


def _live_counts(Z, c, b, W):
    """Oracle: rows with l - max l >= ln tau for one of the 16 components of the block, per (tile, row block)."""
    L = O.canonical_eval(Z, c, b, W)
    K, N = L.shape
    K16, nt = (K + 15) // 16, (N + T - 1) // T
    live = np.zeros((nt * T, K16), dtype=bool)
    hit = (L - L.max(axis=0) >= LN_TAU).T                    # (N, K)
    for rb in range(K16):
        live[:N, rb] = hit[:, 16 * rb:16 * rb + 16].any(axis=1)
    return live.reshape(nt, T, K16).sum(axis=1), L


def _designed_counts(comp, K):
    K16, nt = (K + 15) // 16, (len(comp) + T - 1) // T
    want = np.zeros((nt, K16), dtype=int)
    np.add.at(want, (np.arange(len(comp)) // T, comp // 16), 1)
    return want


def _pass(engine, v, c, b, W):
    engine.tune("resp_skip_log2", v)
    S, sc = engine.estep(c, b, W)
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()]), sc.copy()


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _check(engine, Z, c, b, W, want, num_cu=0):
    """The designed live counts hold (CPU); then skip == oracle (1e-11) == dense (1e-13), scalars and repeats bit-equal."""
    K = len(c)
    counts, L = _live_counts(Z, c, b, W)
    assert np.array_equal(counts, want), (counts, want)
    engine.upload(Z)
    try:
        engine.tune("num_cu", num_cu)
        engine.tune("mid_min_d", 64)                         # K = 33 .. 48 would otherwise take the mid kernel (ROUTING.md)
        plan = engine.plan(K)
        assert plan["kind"] == "fused"
        if num_cu:
            assert plan["workgroups"] * 4 <= len(want)       # every workgroup walks several tiles
        skip, sc_skip = _pass(engine, 60, c, b, W)
        skip2, sc_skip2 = _pass(engine, 60, c, b, W)
        dense, sc_dense = _pass(engine, 0, c, b, W)
        engine.tune("resp_skip_log2", 60)
        engine.estep_async(c, b, W)
        S_a, sc_a = engine.estep_wait()
    finally:
        engine.tune("resp_skip_log2", 60)
        engine.tune("num_cu", 0)
        engine.tune("mid_min_d", 0)
    lse = logsumexp(L, axis=0)
    n, sx, sxx = O.packed_stats(Z, np.exp(L - lse))
    ref = np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)])
    assert _rel(skip, ref) < 1e-11
    assert _rel(skip, dense) < 1e-13
    assert np.array_equal(sc_skip, sc_dense, equal_nan=True)
    assert np.array_equal(skip, skip2) and np.array_equal(sc_skip, sc_skip2, equal_nan=True)
    async_ = np.concatenate([S_a.n.ravel(), S_a.sx.ravel(), S_a.sxx.ravel()])
    assert np.array_equal(async_, skip) and np.array_equal(sc_a, sc_skip, equal_nan=True)


@pytest.mark.parametrize("D,K", SHAPES)
def test_constructed_live_counts(engine, D, K):
    """Row block 0 has 0, 1, 3, 4, 5, 8, 29 and 32 live rows in tiles 0..7; a row is live only in its own block."""
    rng = np.random.default_rng(1000 * D + K)
    mus, c, b, W = _params(rng, D, K, 1.0)
    comp = _components(rng, K)
    Z = np.ascontiguousarray(mus[comp] + rng.standard_normal((len(comp), D)))
    want = _designed_counts(comp, K)
    assert list(want[:, 0]) == BLOCK0_COUNTS and np.all(want.sum(axis=1) == T)
    _check(engine, Z, c, b, W, want)


@pytest.mark.parametrize("D,K", SHAPES)
def test_every_row_live_in_every_block(engine, D, K):
    """Means * 0.01: every mask is 0xFFFFFFFF (the last tile's: its rows below N), all eight groups of every block."""
    rng = np.random.default_rng(2000 * D + K)
    mus, c, b, W = _params(rng, D, K, 0.01)
    N = 4 * T + 5
    Z = np.ascontiguousarray(mus[rng.integers(K, size=N)] + rng.standard_normal((N, D)))
    want = np.full(((N + T - 1) // T, (K + 15) // 16), T)
    want[-1] = N % T
    _check(engine, Z, c, b, W, want)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 4 * 32 + 5])
def test_ragged_row_counts(engine, N):
    """The constructed tiles cut at N: rows past N inside a live tile are never members."""
    D, K = 16, 64
    rng = np.random.default_rng(3000 + N)
    mus, c, b, W = _params(rng, D, K, 1.0)
    comp = _components(rng, K)[::-1][:N].copy()              # reversed: tile 0 has 32 rows of block 0, tile 1 has 29, ...
    Z = np.ascontiguousarray(mus[comp] + rng.standard_normal((N, D)))
    _check(engine, Z, c, b, W, _designed_counts(comp, K))


def test_many_tiles_per_workgroup(engine):
    """Two workgroups ("num_cu" = 1) walk 20 tiles each: the refill across tile boundaries, the last group many times."""
    D, K = 16, 64
    rng = np.random.default_rng(4000)
    mus, c, b, W = _params(rng, D, K, 1.0)
    comp = _components(rng, K, reps=5)[:-7]                  # 40 tiles, the last one ragged
    Z = np.ascontiguousarray(mus[comp] + rng.standard_normal((len(comp), D)))
    _check(engine, Z, c, b, W, _designed_counts(comp, K), num_cu=1)
