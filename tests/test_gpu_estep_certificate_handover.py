"""The certified E-step's row check, evaluated one tile ahead ("E-step certificates"): what moving it from the
front of step 3 to the hand-over behind the previous tile can break.  As in tests/test_gpu_estep_certificate.py every pass runs
twice on the same context state, with mimo_tune "estep_cert" at 1 and at 0 — the second is the skipping kernel, which this
change does not touch — and statistics and scalars must be the same bits; separately they are held against the oracle at that
file's bounds (statistics 1e-11 of the largest entry, the sum of the log-normalisers 1e-12 relative).

  * hand-over across the tiles of one workgroup, and the prefetch past the data: mimo_tune "num_cu" = 1 leaves two workgroups,
    Dz = 14, 15, 16, K = 64 (and K = 49 at Dz = 16: a padded last row block), N = 167 (three tiles each, the last one partial, the
    prefetch two tiles past the end), N = 1, 32, 33 (a workgroup without a tile, one tile, a full tile and a one-row tile);
  * every count of contracted rows a wave can see: five tiles laid out row by row (the table in the test), whose totals of
    mimo_estep_cert_info follow from the construction; with the whole grid (every tile a workgroup's first: the descriptor made in
    front of the loop) and with two workgroups (made at the hand-over);
  * a second reference pass replaces the first: the certified pass after it runs on the new reference's constants.

The file passes on the commit before the check moved, with the same totals: they follow from the rows, not from the kernel."""
import numpy as np
import pytest
from scipy.special import logsumexp

from conftest import rel_err
from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu


def _params(K, D, spread, seed):
    """K Gaussians with precision ~ I, the means `spread` apart along the axes (hundreds of nats between any two)"""
    rng = np.random.default_rng(seed)
    k = np.arange(K)
    mus = np.zeros((K, D))
    mus[k, k % D] = spread * (1 + k // D)
    A = 0.05 * rng.standard_normal((K, D, D))
    W = np.eye(D) + A + A.transpose(0, 2, 1) + 0.1 * np.einsum("kij,klj->kil", A, A)
    return mus, W, -1.0 + 0.1 * rng.standard_normal(K)


def _canonical(mus, W, ch):
    b = np.einsum("kij,kj->ki", W, mus)
    return np.ascontiguousarray(ch - 0.5 * np.einsum("kd,kd->k", b, mus)), np.ascontiguousarray(b), np.ascontiguousarray(W)


def _moved(mus, W, ch, step, seed):
    """a small move of every component: means by 0.02 sigma, precisions by 1 %, peaks by 0.01, `step` times over"""
    rng = np.random.default_rng(seed)
    K, D = mus.shape
    A = 0.005 * step * rng.standard_normal((K, D, D))
    return (mus + 0.02 * step * rng.standard_normal(mus.shape), W * (1.0 + 0.01 * step * rng.uniform(-1, 1, size=(K, 1, 1))) + A + A.transpose(0, 2, 1),
            ch + 0.01 * step * rng.standard_normal(K))


def _flat(S):
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()])


def _oracle(Z, c, b, W):
    L = O.canonical_eval(Z, c, b, W)
    lse = logsumexp(L, axis=0)
    n, sx, sxx = O.packed_stats(Z, np.exp(L - lse))
    return np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)]), float(lse.sum())


@pytest.fixture
def eng(engine):
    engine.tune("resp_skip_log2", 60)
    engine.tune("estep_cert", 1)
    yield engine
    engine.tune("num_cu", 0)
    engine.tune("resp_skip_log2", 60)
    engine.tune("estep_cert", 1)
    engine.set_component_order(None)


def _both(eng, Z, c, b, W):
    """the pass with the certificates and, on the same state, without; both against the oracle -> (kind, rows proven, one-group
    wave-tiles, wave-tiles)"""
    before = eng.estep_cert_info()
    S, sc = eng.estep(c, b, W)
    S, sc = _flat(S).copy(), sc.copy()
    info = eng.estep_cert_info()
    eng.tune("estep_cert", 0)
    S0, sc0 = eng.estep(c, b, W)
    assert eng.estep_cert_info()["kind"] == "plain"
    eng.tune("estep_cert", 1)
    ref, ref_lse = _oracle(Z, c, b, W)
    e_s, e_l = rel_err(S, ref), abs(sc[0] - ref_lse) / abs(ref_lse)
    print("%s: vs oracle %.2e, lse %.2e" % (info["kind"], e_s, e_l))
    assert np.array_equal(S, _flat(S0)) and np.array_equal(sc, sc0, equal_nan=True), info["kind"]
    assert e_s < 1e-11 and e_l < 1e-12
    return (info["kind"], info["proven_rows"] - before["proven_rows"], info["one_group"] - before["one_group"],
            info["wave_tiles"] - before["wave_tiles"])


def _start(eng, Z, order, c, b, W):
    """upload, order, and the two passes the partition has to stand for: plain, then the reference pass"""
    eng.upload(Z)
    eng.set_component_order(order)
    K = len(order)
    assert eng.plan(K)["kind"] == "fused" and eng.plan(K)["component_order"]
    kinds = (_both(eng, Z, c, b, W)[0], _both(eng, Z, c, b, W)[0])
    assert kinds == ("plain", "reference"), kinds
    assert eng.estep_cert_info()["valid"]


HANDOVER = [(D, 64, N) for D in (14, 15, 16) for N in (167, 1, 32, 33)] + [(16, 49, 167)]


@pytest.mark.parametrize("D,K,N", HANDOVER)
def test_hand_over_across_the_tiles_of_a_workgroup(eng, D, K, N):
    """Two workgroups: each runs its tiles one after the other, the check of the next tile made at the end of the one before; the
    certificate prefetch runs two tiles past the data."""
    eng.tune("num_cu", 1)
    mus, W, ch = _params(K, D, 40.0, D + K)
    rng = np.random.default_rng(N)
    # (at most 33 rows: from the D clusters nearest the origin.  The canonical form cancels terms of |mu|^2 / 2, up to 12 800 nats at
    # the outermost clusters, and the 1e-12 of the sum of log-normalisers is then not a bound one or two rows can be held to —
    # the plain pass misses it there as well)
    Z = np.ascontiguousarray(mus[rng.integers(K if N > 33 else D, size=N)] + rng.standard_normal((N, D)))
    order = np.random.default_rng(D + N).permutation(K).astype(np.int32)
    _start(eng, Z, order, *_canonical(mus, W, ch))
    tiles = -(-N // 32)
    for step in (1, 2):
        kind, proven, one, all_wt = _both(eng, Z, *_canonical(*_moved(mus, W, ch, step, 7 * step)))
        assert kind == "certified" and all_wt == 4 * tiles
        assert proven > 0.9 * N and one >= 3 * (N // 32)


# The five tiles, D = 16, K = 64, the identity order (component k in row block k >> 4), the clusters 80 sigma apart.  Component 50
# (block 3) is moved 42 sigma after the reference pass: the bound on its own rows' maximum falls by 2 d^2 / 2 + d^2 / 2 = 2 600 nats
# and its 32 rows are unproven, so every wave has to contract them; the bound of its class on every other row rises by d^2 / 2 =
# 900 nats to about 900 - 80^2 / 4 = -700, which still lies under every other row's own maximum - 42 (DESIGN, the test per row).
#   tile  rows                                            contracted rows of waves 0..3    on one column group
#   1     16 of block 0 + 16 of block 1                   16, 16, 0, 0                     4
#   2     17 of block 0 + 15 of block 1                   17, 15, 0, 0                     3 (wave 0 takes the two-group branch)
#   3     32 of block 2                                   0, 0, 32, 0                      3 (the empty-need slot rule in three waves)
#   4     1 of block 3 + 31 of component 50               31, 31, 31, 32                   0
#   5     16 of block 0 + 1 of component 50 + 15 of block 1    17, 16, 1, 1                3
# (Tile 5 is a full tile, so besides the 16 proven rows of block 0 and the unproven row it holds 15 more rows; they are proven rows
# of block 1, which puts wave 1 at exactly 16 with an unproven row among them and leaves waves 2 and 3 at 1.)
def _five_tiles():
    b0, b1, b2 = np.arange(16), 16 + np.arange(16), 32 + np.arange(16)
    return np.concatenate([b0, b1,
                           b0, [3], b1[:15],
                           b2, b2,
                           [60], np.full(31, 50),
                           b0, [50], b1[:15]])


@pytest.mark.parametrize("num_cu", [0, 1])
def test_every_count_of_contracted_rows(eng, num_cu):
    D, K = 16, 64
    eng.tune("num_cu", num_cu)
    mus, W, ch = _params(K, D, 80.0, 5)
    comp = _five_tiles()
    N = len(comp)
    assert N == 160
    Z = np.ascontiguousarray(mus[comp] + np.random.default_rng(8).standard_normal((N, D)))
    _start(eng, Z, np.arange(K, dtype=np.int32), *_canonical(mus, W, ch))
    kind, proven, one, all_wt = _both(eng, Z, *_canonical(mus, W, ch))
    # nothing moved: every row proven.  Tiles 1 .. 5 on one group: 4, 3, 3, 3 (32 rows of block 3: waves 0 - 2 hold none), 4 (16, 15, 0, 1)
    assert (kind, proven, one, all_wt) == ("certified", 160, 17, 20), (kind, proven, one, all_wt)
    moved = mus.copy()
    moved[50] += 42.0 / np.sqrt(D)
    kind, proven, one, all_wt = _both(eng, Z, *_canonical(moved, W, ch))
    assert (kind, proven, one, all_wt) == ("certified", 128, 13, 20), (kind, proven, one, all_wt)


def test_a_second_reference_pass_replaces_the_first(eng):
    """reference -> certified -> another resp_skip_log2 and back, a pass at each: the certificates are dropped and, the partition
    having stood, the pass is the next reference pass at once (the policy has no plain pass here) -> certified on the second
    reference, a different posterior.  A host-side block left over from the first reference would give the wrong constants."""
    D, K, N = 16, 64, 167
    eng.tune("num_cu", 1)
    mus, W, ch = _params(K, D, 40.0, 21)
    rng = np.random.default_rng(2)
    Z = np.ascontiguousarray(mus[rng.integers(K, size=N)] + rng.standard_normal((N, D)))
    _start(eng, Z, np.arange(K, dtype=np.int32), *_canonical(mus, W, ch))
    assert _both(eng, Z, *_canonical(*_moved(mus, W, ch, 1, 3)))[0] == "certified"
    eng.tune("resp_skip_log2", 50)
    assert _both(eng, Z, *_canonical(mus, W, ch))[0] == "reference"
    eng.tune("resp_skip_log2", 60)
    # the second reference: precisions 1.5 to 2.5 times the first's, means a quarter sigma elsewhere
    rng = np.random.default_rng(4)
    mus2, W2, ch2 = mus + 0.25 * rng.standard_normal(mus.shape), W * rng.uniform(1.5, 2.5, size=(K, 1, 1)), ch + 0.5
    assert _both(eng, Z, *_canonical(mus2, W2, ch2))[0] == "reference"
    kind, proven, one, all_wt = _both(eng, Z, *_canonical(*_moved(mus2, W2, ch2, 1, 6)))
    assert kind == "certified" and proven > 0.9 * N and all_wt == 4 * 6
    kind, proven, one, all_wt = _both(eng, Z, *_canonical(*_moved(mus2, W2, ch2, 2, 7)))
    assert kind == "certified" and proven > 0.9 * N
