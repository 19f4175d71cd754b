"""Per-row certificates of the fused mean-field E-step (mimo_tune "estep_cert"; DESIGN section 4, "E-step certificates") on the
GPU.  Every pass is run twice on the same context state, with the key at 1 and at 0 — the second is the skipping kernel as it
was — and the statistics and scalars must be the same bits; separately they are held against the oracle at the bounds of
tests/test_gpu_estep_seed.py (statistics 1e-11 of the largest entry, the sum of the log-normalisers 1e-12 relative).  Which
kind of pass ran, and what it proved, is read from mimo_estep_cert_info.  Dz = 14, 15, 16 (the three skipping instantiations),
K = 64; N = 37 (one full tile and a partial one), 224 (whole tiles), 1285 (forty tiles and a ragged end)."""
import numpy as np
import pytest
from scipy.special import logsumexp

from conftest import rel_err
from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

K = 64
DIMS = [14, 15, 16]
ROWS = [37, 32 * 7, 32 * 40 + 5]


def _params(D, spread, seed):
    """K Gaussians with precision ~ I, the means `spread` apart along the axes (40: separated by hundreds of nats; 0.5: all on
    top of each other)"""
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
    D = mus.shape[1]
    A = 0.005 * step * rng.standard_normal((K, D, D))
    return (mus + 0.02 * step * rng.standard_normal(mus.shape), W * (1.0 + 0.01 * step * rng.uniform(-1, 1, size=(K, 1, 1))) + A + A.transpose(0, 2, 1),
            ch + 0.01 * step * rng.standard_normal(K))


def _rows(mus, N, seed, only=None):
    rng = np.random.default_rng(seed)
    comp = rng.integers(K, size=N) if only is None else np.full(N, only)
    return np.ascontiguousarray(mus[comp] + rng.standard_normal((N, mus.shape[1]))), comp


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
    engine.tune("resp_skip_log2", 60)
    engine.tune("estep_cert", 1)
    engine.set_component_order(None)


def _both(eng, c, b, W, asynchronous=False):
    """the pass with the certificates and, on the same state, without: (bits equal, kind, rows proven, one-group wave-tiles,
    wave-tiles, statistics, scalars)"""
    before = eng.estep_cert_info()
    if asynchronous:
        eng.estep_async(c, b, W)
        S, sc = eng.estep_wait()
    else:
        S, sc = eng.estep(c, b, W)
    S, sc = _flat(S).copy(), sc.copy()
    info = eng.estep_cert_info()
    eng.tune("estep_cert", 0)
    S0, sc0 = eng.estep(c, b, W)
    assert eng.estep_cert_info()["kind"] == "plain"
    eng.tune("estep_cert", 1)
    same = np.array_equal(S, _flat(S0)) and np.array_equal(sc, sc0, equal_nan=True)
    return (same, info["kind"], info["proven_rows"] - before["proven_rows"], info["one_group"] - before["one_group"],
            info["wave_tiles"] - before["wave_tiles"], S, sc)


def _start(eng, Z, order, c, b, W):
    """upload, order, and the two passes the partition has to stand for: plain, then the reference pass"""
    eng.upload(Z)
    eng.set_component_order(order)
    assert eng.plan(K)["kind"] == "fused" and eng.plan(K)["component_order"]
    first = _both(eng, c, b, W)
    second = _both(eng, c, b, W)
    assert first[0] and second[0]
    assert (first[1], second[1]) == ("plain", "reference"), (first[1], second[1])
    assert eng.estep_cert_info()["valid"]


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_separated_clusters(eng, D, N):
    """Reference pass, then three certified passes under small moves: the same bits as without, rows proven, wave-tiles on one
    column group; the oracle's statistics."""
    mus, W, ch = _params(D, 40.0, D)
    Z, _ = _rows(mus, N, N)
    order = np.random.default_rng(D + N).permutation(K).astype(np.int32)
    _start(eng, Z, order, *_canonical(mus, W, ch))
    tiles = -(-N // 32)
    for step in (1, 2, 3):
        c, b, Wc = _canonical(*_moved(mus, W, ch, step, 7 * step))
        same, kind, proven, one, all_wt, S, sc = _both(eng, c, b, Wc, asynchronous=step == 2)
        ref, ref_lse = _oracle(Z, c, b, Wc)
        print("Dz=%d N=%d step %d: %s, %d of %d rows proven, %d of %d wave-tiles on one group; vs oracle %.2e, lse %.2e"
              % (D, N, step, kind, proven, N, one, all_wt, rel_err(S, ref), abs(sc[0] - ref_lse) / abs(ref_lse)))
        assert same and kind == "certified"
        assert all_wt == 4 * tiles and proven > 0.9 * N
        assert one >= 3 * (N // 32)              # of a whole tile's four waves at most one holds 17 of its rows or more
        assert rel_err(S, ref) < 1e-11
        assert abs(sc[0] - ref_lse) < 1e-12 * abs(ref_lse)
        S2, sc2 = eng.estep(c, b, Wc)            # a repeat
        assert np.array_equal(_flat(S2), S) and np.array_equal(sc2, sc, equal_nan=True)


@pytest.mark.parametrize("D,N", [(14, 37), (15, 32 * 7), (16, 32 * 40 + 5)])
def test_overlapping_clusters_prove_nothing(eng, D, N):
    mus, W, ch = _params(D, 0.5, D)
    Z, _ = _rows(mus, N, N)
    _start(eng, Z, np.arange(K, dtype=np.int32), *_canonical(mus, W, ch))
    c, b, Wc = _canonical(*_moved(mus, W, ch, 1, 3))
    same, kind, proven, one, all_wt, S, sc = _both(eng, c, b, Wc)
    assert same and kind == "certified" and proven == 0 and one == 0 and all_wt == 4 * -(-N // 32)
    ref, ref_lse = _oracle(Z, c, b, Wc)
    assert rel_err(S, ref) < 1e-11 and abs(sc[0] - ref_lse) < 1e-12 * abs(ref_lse)


@pytest.mark.parametrize("D,N", [(14, 32 * 7), (15, 32 * 40 + 5), (16, 37)])
def test_a_large_move_of_one_mean_unproves_its_rows(eng, D, N):
    mus, W, ch = _params(D, 40.0, D)
    Z, comp = _rows(mus, N, N + 1)
    _start(eng, Z, np.arange(K, dtype=np.int32), *_canonical(mus, W, ch))
    c, b, Wc = _canonical(mus, W, ch)
    same, kind, proven_all, _, _, _, _ = _both(eng, c, b, Wc)
    assert same and kind == "certified" and proven_all == N
    moved = mus.copy()
    moved[5] += 30.0 / np.sqrt(D)                                   # 30 sigma away: the bound on its own rows' maximum is gone
    c, b, Wc = _canonical(moved, W, ch)
    same, kind, proven, _, _, S, sc = _both(eng, c, b, Wc)
    assert same and kind == "certified"
    assert proven <= N - int((comp == 5).sum()) and proven < proven_all
    ref, ref_lse = _oracle(Z, c, b, Wc)
    assert rel_err(S, ref) < 1e-11 and abs(sc[0] - ref_lse) < 1e-12 * abs(ref_lse)


@pytest.mark.parametrize("D,N", [(14, 32 * 40 + 5), (15, 37), (16, 32 * 7)])
def test_all_rows_from_one_cluster_take_the_two_group_branch(eng, D, N):
    """Every row proven and in the block of component 21: that wave needs all 32 rows of a tile and runs the two column groups,
    the other three need only the rows past N — one group where those are at most 16."""
    mus, W, ch = _params(D, 40.0, D)
    Z, _ = _rows(mus, N, N + 2, only=21)
    _start(eng, Z, np.arange(K, dtype=np.int32), *_canonical(mus, W, ch))
    c, b, Wc = _canonical(*_moved(mus, W, ch, 1, 5))
    same, kind, proven, one, all_wt, S, sc = _both(eng, c, b, Wc)
    tail = N % 32
    assert same and kind == "certified" and proven == N
    assert one == 3 * (N // 32 + (1 if tail >= 16 else 0)) and all_wt == 4 * -(-N // 32)
    ref, ref_lse = _oracle(Z, c, b, Wc)
    assert rel_err(S, ref) < 1e-11 and abs(sc[0] - ref_lse) < 1e-12 * abs(ref_lse)


@pytest.mark.parametrize("D,N", [(14, 37), (16, 32 * 40 + 5)])
def test_a_permutation_of_slots_and_blocks_keeps_the_certificates(eng, D, N):
    mus, W, ch = _params(D, 40.0, D)
    Z, _ = _rows(mus, N, N + 3)
    order = np.random.default_rng(N).permutation(K).astype(np.int32)
    _start(eng, Z, order, *_canonical(mus, W, ch))
    rng = np.random.default_rng(D)
    blocks = [rng.permutation(order[16 * i:16 * i + 16]) for i in rng.permutation(4)]      # the same four sets, elsewhere
    eng.set_component_order(np.concatenate(blocks).astype(np.int32))
    c, b, Wc = _canonical(*_moved(mus, W, ch, 1, 9))
    same, kind, proven, one, _, S, sc = _both(eng, c, b, Wc)
    assert same and kind == "certified" and proven > 0.9 * N and one > 0
    ref, ref_lse = _oracle(Z, c, b, Wc)
    assert rel_err(S, ref) < 1e-11 and abs(sc[0] - ref_lse) < 1e-12 * abs(ref_lse)


def test_what_drops_the_certificates(eng):
    """Another partition: the next pass is plain, the one after it the new reference pass.  A new upload: the same.  Another
    resp_skip_log2: the partition has stood, so the next pass is the reference pass.  Sixteen certified passes: renewed."""
    D, N = 16, 32 * 7
    mus, W, ch = _params(D, 40.0, D)
    Z, _ = _rows(mus, N, 11)
    c, b, Wc = _canonical(mus, W, ch)
    order = np.arange(K, dtype=np.int32)
    _start(eng, Z, order, c, b, Wc)

    def kinds(n):
        out = []
        for _ in range(n):
            same, kind = _both(eng, c, b, Wc)[:2]
            assert same
            out.append(kind)
        return out

    assert kinds(2) == ["certified", "certified"]
    other = order.copy()
    other[[3, 40]] = other[[40, 3]]                                 # components 3 and 40 trade row blocks
    eng.set_component_order(other)
    assert kinds(3) == ["plain", "reference", "certified"]
    eng.upload(Z)
    eng.set_component_order(other)
    assert not eng.estep_cert_info()["valid"]
    assert kinds(3) == ["plain", "reference", "certified"]
    eng.tune("resp_skip_log2", 50)
    assert kinds(2) == ["reference", "certified"]
    eng.tune("resp_skip_log2", 60)
    assert kinds(2) == ["reference", "certified"]
    assert kinds(16) == 15 * ["certified"] + ["reference"]
    eng.estep(c[:48], b[:48], Wc[:48])                              # another K drops the order, and with it the route
    assert eng.estep_cert_info()["kind"] == "plain"


def test_rows_with_nan_keep_their_route(eng):
    D, N = 16, 32 * 7
    mus, W, ch = _params(D, 40.0, D)
    Z, _ = _rows(mus, N, 13)
    Z[[5, 100]] = np.nan
    c, b, Wc = _canonical(mus, W, ch)
    eng.upload(Z)
    eng.set_component_order(np.arange(K, dtype=np.int32))
    for _ in range(3):
        same, kind = _both(eng, c, b, Wc)[:2]
        assert same and kind == "plain"
