"""mimo_host_block_order on the CPU: the slot order the mean-field driver hands to the fused pass (mimo_set_component_order).
Properties of the partition, the rejections, a sanitizer run of a stand-alone program, and the model of what the order buys:
live row blocks per row and groups of four live rows per (tile, row block) of the fused kernel's responsibility skip, on the
benchmark's own data recipe and start."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mimo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_order(means, mass, block=16):
    means, mass = np.ascontiguousarray(means, dtype=float), np.ascontiguousarray(mass, dtype=float)
    K, D = means.shape
    order = np.full(K, -1, dtype=np.int32)
    rc = _lib.load().mimo_host_block_order(K, D, means.ctypes.data, mass.ctypes.data, block, order.ctypes.data)
    assert rc == 0, rc
    return order


def blocks_of(order):
    """block of every component"""
    blk = np.empty(len(order), dtype=int)
    blk[order] = np.arange(len(order)) // 16
    return blk


def partition(order):
    return {frozenset(int(k) for k in order[s:s + 16]) for s in range(0, len(order), 16)}


def _random_posterior(rng, K, D, n_centres):
    centres = rng.normal(0.0, 6.0, size=(n_centres, D))
    means = centres[rng.integers(n_centres, size=K)] + 0.05 * rng.standard_normal((K, D))
    mass = np.where(rng.random(K) < 0.3, 1e-2, 100.0 + 1000.0 * rng.random(K))
    return means, mass


@pytest.mark.parametrize("K,D", [(1, 3), (16, 16), (17, 16), (40, 14), (64, 16), (256, 8)])
def test_permutation_and_repeats(K, D):
    rng = np.random.default_rng(K + D)
    means, mass = _random_posterior(rng, K, D, max(1, K // 2))
    order = block_order(means, mass)
    assert sorted(order) == list(range(K))
    assert np.array_equal(order, block_order(means, mass))
    assert np.array_equal(order, block_order(means.copy(), mass.copy()))


def test_copies_share_a_block():
    """Two copies of the same means land in one block, wherever the identity has them."""
    rng = np.random.default_rng(5)
    K, D = 64, 16
    means = rng.normal(0.0, 6.0, size=(K, D))
    mass = np.full(K, 500.0)
    for a, b in [(0, 63), (3, 17), (20, 40), (31, 32)]:
        means[b] = means[a]
    blk = blocks_of(block_order(means, mass))
    for a, b in [(0, 63), (3, 17), (20, 40), (31, 32)]:
        assert blk[a] == blk[b] and a // 16 != b // 16


def test_separated_pairs_fill_four_blocks():
    """32 well-separated pairs of equal mass, the partners 32 apart in arrival order: four blocks of 8 whole pairs."""
    rng = np.random.default_rng(6)
    D = 16
    centres = 50.0 * rng.standard_normal((32, D))
    means = np.concatenate([centres, centres + 0.01 * rng.standard_normal((32, D))])
    blk = blocks_of(block_order(means, np.full(64, 1000.0)))
    assert np.array_equal(blk[:32], blk[32:])
    assert list(np.bincount(blk, minlength=4)) == [16, 16, 16, 16]


def test_fillers_and_padding():
    """Components below mass 1 take the slots the others leave, in index order: inside every block the components with mass
    come first.  K = 40: the order names the 40 real slots only (16 + 16 + 8), the padding slots 40 .. 47 are not in it."""
    rng = np.random.default_rng(8)
    K, D = 40, 14
    means = rng.normal(0.0, 6.0, size=(K, D))
    mass = np.full(K, 300.0)
    fillers = [1, 5, 22, 39]
    mass[fillers] = 0.25
    order = block_order(means, mass)
    assert sorted(order) == list(range(K))
    assert [int(k) for k in order if k in fillers] == fillers
    assert len(order) == K
    for s in (0, 16, 32):
        is_filler = [int(k) in fillers for k in order[s:s + 16]]
        assert is_filler == sorted(is_filler), (s, order[s:s + 16])                   # actives, then fillers
    # 36 components with mass in blocks of 16, 16 and 8 slots: no block is left without one
    assert all(any(int(k) not in fillers for k in order[s:s + 16]) for s in (0, 16, 32))


def test_permuting_the_input_permutes_the_partition():
    rng = np.random.default_rng(9)
    K, D = 64, 16
    means, mass = _random_posterior(rng, K, D, 24)
    mass = mass * (1.0 + 0.1 * rng.random(K))                       # no two clusters of equal mass
    p = rng.permutation(K)                                          # new index i holds old component p[i]
    part = partition(block_order(means, mass))
    part_p = partition(block_order(means[p], mass[p]))
    active = set(np.flatnonzero(mass >= 1.0))
    # the fillers' slots follow their indices; the clusters of the others must not
    assert {frozenset(k for k in blk if k in active) for blk in part} - {frozenset()} == \
        {frozenset(int(p[i]) for i in blk if p[i] in active) for blk in part_p} - {frozenset()}


def test_rejections():
    lib = _lib.load()
    K, D = 64, 16
    means, mass, order = np.ones((K, D)), np.full(K, 5.0), np.zeros(K, dtype=np.int32)
    m, w, o = means.ctypes.data, mass.ctypes.data, order.ctypes.data
    assert lib.mimo_host_block_order(0, D, m, w, 16, o) == _lib.E_INVALID
    assert lib.mimo_host_block_order(-3, D, m, w, 16, o) == _lib.E_INVALID
    assert lib.mimo_host_block_order(K, 0, m, w, 16, o) == _lib.E_INVALID
    for block in (0, 8, 15, 17, 32):
        assert lib.mimo_host_block_order(K, D, m, w, block, o) == _lib.E_INVALID
    assert lib.mimo_host_block_order(K, D, None, w, 16, o) == _lib.E_INVALID
    assert lib.mimo_host_block_order(K, D, m, None, 16, o) == _lib.E_INVALID
    assert lib.mimo_host_block_order(K, D, m, w, 16, None) == _lib.E_INVALID
    assert lib.mimo_host_block_order(257, 1, m, w, 16, o) == _lib.E_UNSUPPORTED
    for bad in (np.nan, np.inf, -np.inf):
        for arr, idx in ((means, (63, 15)), (mass, (63,))):
            keep = arr[idx]
            arr[idx] = bad
            assert lib.mimo_host_block_order(K, D, m, w, 16, o) == _lib.E_INVALID
            arr[idx] = keep
    assert lib.mimo_host_block_order(K, D, m, w, 16, o) == 0


def test_block_order_under_asan_ubsan(tmp_path):
    """K = 1, 16, 17, 64, 256 in a stand-alone program with its own main: nothing is loaded into this process."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "block_order_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-mavx2", "-mfma", "-pthread", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # is the sanitizer runtime there?  An empty program decides that, so no error of the real build can hide as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([hipcc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    build = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tests", "block_order_check.cpp"),
                                              os.path.join(ROOT, "mimo_amd", "csrc", "mimo_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "block order ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]


class _Recorder:
    """what an engine sees of the hook"""

    def __init__(self):
        self.calls = []

    def set_component_order(self, order):
        self.calls.append(None if order is None else np.array(order))


def test_sharded_engine_passes_the_order_through():
    from mimo_amd.sharded import ShardedEngine
    sh = object.__new__(ShardedEngine)                              # (no process group: only the pass-through is exercised)
    sh.inner = _Recorder()
    order = np.arange(32, dtype=np.int32)[::-1]
    sh.set_component_order(order)
    sh.set_component_order(None)
    assert np.array_equal(sh.inner.calls[0], order) and sh.inner.calls[1] is None
    sh.inner = object()                                             # an engine without the call: nothing happens
    sh.set_component_order(order)


@pytest.mark.parametrize("K,expect", [(40, True), (16, False)])
def test_driver_sets_the_order_before_the_pass(K, expect):
    """meanfield_iteration hands the function's order to the engine before estep_async, and leaves K <= 16 (one row block) alone."""
    from oracle_engine import OracleEngine
    from mimo_amd.distributions import (Dirichlet, CategoricalWithDirichlet, StackedNormalWisharts, StackedGaussiansWithNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfGaussians

    class Eng(OracleEngine):
        def __init__(self):
            super().__init__()
            self.log = []

        def set_component_order(self, order):
            self.log.append(("order", None if order is None else np.array(order)))

        def estep_async(self, c, b, W):
            self.log.append(("pass", None))
            self._out = self.estep(c, b, W)

        def estep_wait(self):
            return self._out

    rng = np.random.default_rng(K)
    D, N = 3, 600
    X = rng.normal(0.0, 4.0, size=(8, D))[rng.integers(8, size=N)] + 0.3 * rng.standard_normal((N, D))
    eng = Eng()
    eng.upload(X)
    prior = StackedNormalWisharts(K, D, np.zeros((K, D)), 1e-2 * np.ones(K), np.stack(K * [np.eye(D)]), (D + 1.) * np.ones(K) + 1e-8)
    model = BayesianMixtureOfGaussians(CategoricalWithDirichlet(K, Dirichlet(K, np.ones(K))),
                                       StackedGaussiansWithNormalWisharts(K, D, prior, engine=eng), engine=eng)
    S = eng.label_stats(rng.integers(0, K, size=N), K)
    for _ in range(2):
        S, _ = model.meanfield_iteration(eng, S, sample_likelihood=False)
    kinds = [k for k, _ in eng.log]
    if expect:
        assert kinds == ["order", "pass", "order", "pass"]
        assert all(sorted(o) == list(range(K)) for k, o in eng.log if k == "order")
    else:
        assert kinds == ["pass", "pass"]


# ---- the model: what the fused kernel's responsibility skip contracts under an order -------------------------------------
T, GROUP, LN_TAU = 32, 4, -60 * np.log(2.0)


def skip_cost(L, order):
    """(live row blocks per row, mean groups per (tile, row block), mean over the tiles of the largest block's groups) of the
    log-densities L (K, N) with component order[s] in slot s: a row is live in a block when one of its 16 weights, relative
    to the row's largest, reaches 2^-60; a wave contracts its block's live rows of a 32-row tile four at a time."""
    K, N = L.shape
    hit = (L - L.max(axis=0) >= LN_TAU)[order]                      # slot-major
    live = np.stack([hit[s:s + 16].any(axis=0) for s in range(0, K, 16)], axis=1)     # (N, blocks)
    counts = live[:N // T * T].reshape(N // T, T, -1).sum(axis=1)
    groups = -(-counts // GROUP)
    return live.sum(axis=1).mean(), groups.mean(), groups.max(axis=1).mean()


def _log_densities(X, c, b, W):
    """O.canonical_eval through BLAS: l[k, n] = c_k + b_k . x_n - x_n' W_k x_n / 2 (the oracle's einsum takes 1.3 s on these rows)"""
    return np.stack([c[k] + X @ b[k] - 0.5 * np.einsum("nd,nd->n", X @ W[k], X) for k in range(len(c))])


def _packed_stats(X, R):
    """O.packed_stats through BLAS"""
    return R.sum(axis=1), R @ X, np.stack([(X * r[:, None]).T @ X for r in R])


def test_model_of_the_benchmark_fit():
    """24 576 rows of bench.make_data (c2: D = 16, K = 64) from the benchmark's random hard-label start, 12 iterations of the
    public driver on the CPU oracle.  Under the function's order: from iteration 8 at most 1.05 live blocks per row and at
    most 2.5 groups per (tile, row block) — the identity has 1.2 - 1.3 and 2.8 - 3.0 there — and in every iteration no
    more groups than the identity."""
    import bench
    from oracle import mimo_oracle as O
    from oracle_engine import OracleEngine
    from scipy.special import logsumexp
    from mimo_amd.distributions import native_sweep
    from mimo_amd.engine import SuffStats
    from mimo_amd.mixtures.gmm import _component_stats

    N, D, K = 24576, 16, 64
    X = bench.make_data(N, D, K, seed=1337, device="cpu").numpy()
    eng = OracleEngine()
    eng.upload(X)
    model = bench.build_model(bench.CONFIGS["c2"], eng)
    S = eng.label_stats(np.random.default_rng(4242).integers(0, K, size=N).astype(np.int32), K)
    identity = np.arange(K)
    rows = []
    for it in range(1, 13):
        fused = native_sweep.gmm_vi_sweep(model.gating, model.components, _component_stats(S, model.components), S.gating_counts)
        assert fused is not None
        (c, b, W), bound = fused
        order = bound.block_order
        assert order is not None and sorted(order) == list(range(K))
        L = _log_densities(X, c, b, W)
        if it == 1:                                                 # the two shortcuts against the oracle, on a few rows
            Ls = O.canonical_eval(X[:256], c, b, W)
            assert np.allclose(L[:, :256], Ls, rtol=1e-12, atol=1e-9)
            Rs = np.exp(Ls - logsumexp(Ls, axis=0))
            assert all(np.allclose(x, y, rtol=1e-12, atol=1e-9) for x, y in zip(_packed_stats(X[:256], Rs), O.packed_stats(X[:256], Rs)))
        rows.append((it, skip_cost(L, identity), skip_cost(L, order)))
        S = SuffStats(*_packed_stats(X, np.exp(L - logsumexp(L, axis=0))))      # (what eng.estep(c, b, W) returns)
    for it, ident, ordered in rows:
        print("iteration %2d  identity: %.3f live, %.3f groups (slowest %.3f)   ordered: %.3f live, %.3f groups (slowest %.3f)"
              % ((it,) + ident + ordered))
    for it, ident, ordered in rows:
        assert ordered[1] <= ident[1], (it, ident, ordered)
        if it >= 8:
            assert ordered[0] <= 1.05 and ordered[1] <= 2.5, (it, ident, ordered)
            assert ident[0] >= 1.15 and ident[1] >= 2.7, (it, ident)
