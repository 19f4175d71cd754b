"""The certified E-step's proven waves ("E-step certificates", the proven wave): a wave whose eight rows are
all proven normalises each row over its live row block alone, two slots per lane.  As in
tests/test_gpu_estep_certificate_handover.py every pass runs twice on the same context state, with mimo_tune "estep_cert" at 1
and at 0 — the second is the skipping kernel, which the path does not touch — and statistics and both scalars must be the same
bits.  The four running totals are held against a host model of the row check (the certificates from the reference pass's
log-densities, the table of mimo_host_estep_certificate), which is also what says where the path fires.

K = 64, Dz = 14 and 16, N = 32 * 5 + 11: five full tiles and a ragged one, the clusters 80 sigma apart, the identity order.  A row
drawn at a cluster is proven; a row placed where two clusters of different row blocks are equally likely is live in both blocks
and never proven.  Every case lays out ONE tile of interest; each wave of every other tile holds one such row, so that the new
total counts the waves of that tile alone:

  1  every wave of the tile proven (16 rows of block 0, 16 of block 1);
  2  one wave holds a row live in two blocks and takes the eight-slot path, the other three take the new one;
  3  the ragged last tile: 11 proven rows, wave 0 on the new path, wave 1 with rows past N (unproven) on the old one;
  4  the eight rows of every wave lie in four different row blocks;
  5  20 rows of block 0 and 12 of block 1: wave 0 contracts more than 16 rows (the two-group code), all four normalising
     waves are proven;
  6  (in every case) a second certified pass after the posterior has moved.

With two workgroups (mimo_tune "num_cu" = 1: the descriptor made at the hand-over, three tiles each) and, at Dz = 16, with the
whole grid (made in front of the loop)."""
import numpy as np
import pytest

from test_block_order_cpu import _log_densities
from test_estep_certificate_cpu import EPS, LN_TAU, bounds_built, certificates, native
from test_gpu_estep_certificate_handover import _canonical, _flat, _moved, _params

pytestmark = pytest.mark.gpu

K, N, T = 64, 32 * 5 + 11, 32
TILES = -(-N // T)
BLK = np.arange(K) // 16
# the tile of interest of each case, and the (tile, wave) pairs the construction makes proven there
AT = {1: 1, 2: 2, 3: 5, 4: 4, 5: 0}
PROVEN_WAVES = {1: (0, 1, 2, 3), 2: (0, 1, 3), 3: (0,), 4: (0, 1, 2, 3), 5: (0, 1, 2, 3)}


def _between(canon, k1, k2):
    """the point of the segment from the centre of k1 to that of k2 where the two log-densities are equal (bisection)"""
    c, b, W = canon
    mu1, mu2 = np.linalg.solve(W[k1], b[k1]), np.linalg.solve(W[k2], b[k2])

    def gap(t):
        z = mu1 + t * (mu2 - mu1)
        l1, l2 = (c[k] + b[k] @ z - 0.5 * z @ W[k] @ z for k in (k1, k2))
        return l1 - l2

    lo, hi = 0.0, 1.0
    assert gap(lo) > 0.0 > gap(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gap(mid) > 0.0 else (lo, mid)
    return mu1 + lo * (mu2 - mu1)


def _unproven_wave(D, w, rows=8):
    """rows of a wave with one row live in two blocks: components of block w, and a pair (k, k + D) of two row blocks: neighbours
    on one axis (_params), 40 sigma from the point between them, which every other component is at least 120 sigma away from"""
    k = (5, 20, 40, 45)[w]
    assert BLK[k] != BLK[k + D]
    return [16 * w + i for i in range(rows - 1)] + [(k, k + D)]


def _layout(case, D):
    """per tile the list of rows: k (drawn at component k) or (k1, k2) (equally likely under both)"""
    tiles = [sum((_unproven_wave(D, w) for w in range(4)), []) for _ in range(TILES - 1)] + [_unproven_wave(D, 0) + _unproven_wave(D, 1, 3)]
    b = [list(range(16 * i, 16 * i + 16)) for i in range(4)]
    if case == 1:
        tiles[AT[1]] = b[0] + b[1]
    elif case == 2:
        tiles[AT[2]] = b[2] + b[3][:7] + [(3, 3 + D)] + b[3][8:]
    elif case == 3:
        tiles[AT[3]] = b[1][:11]
    elif case == 4:
        tiles[AT[4]] = sum(([0 + w, 16 + w, 32 + w, 48 + w, 4 + w, 20 + w, 36 + w, 52 + w] for w in range(4)), [])
    else:
        tiles[AT[5]] = b[0] + b[0][:4] + b[1][:12]
    rows = sum(tiles, [])
    assert len(rows) == N and all(len(t) == T for t in tiles[:-1])
    return rows


def _data(case, D, mus, canon):
    rng = np.random.default_rng(100 * D + case)
    return np.ascontiguousarray([_between(canon, *r) if isinstance(r, tuple) else mus[r] + rng.standard_normal(D) for r in _layout(case, D)])


def _host_model(Z, ref, cur):
    """the row check of a certified pass on the host -> (rows proven, wave-tiles on one column group, wave-tiles, the (tiles, 4)
    mask of waves whose eight rows are all proven, the (tiles, 4) counts of rows each wave contracts)"""
    cert = certificates(_log_densities(Z, *ref), BLK)
    U, M = bounds_built(cert, native(ref, cur)[2])
    prov, own = np.zeros(TILES * T, dtype=bool), np.zeros(TILES * T, dtype=int)
    prov[:N], own[:N] = U - M <= LN_TAU - EPS, BLK[cert[0]]           # (a row past N is unproven)
    prov, own = prov.reshape(TILES, T), own.reshape(TILES, T)
    need = np.stack([(~prov).sum(axis=1) + (prov & (own == w)).sum(axis=1) for w in range(4)], axis=1)
    return int(prov.sum()), int((need <= 16).sum()), 4 * TILES, prov.reshape(TILES, 4, 8).all(axis=2), need


@pytest.fixture
def eng(engine):
    engine.tune("resp_skip_log2", 60)
    engine.tune("estep_cert", 1)
    yield engine
    engine.tune("num_cu", 0)
    engine.tune("resp_skip_log2", 60)
    engine.tune("estep_cert", 1)
    engine.set_component_order(None)


def _totals(eng):
    info = eng.estep_cert_info()
    return np.array([info["proven_rows"], info["one_group"], info["wave_tiles"], eng.estep_cert_proven_waves()])


def _both(eng, canon):
    """the pass with the certificates and, on the same state, with the key at 0: the same bits -> (kind, what the four totals rose by)"""
    before = _totals(eng)
    S, sc = eng.estep(*canon)
    S, sc = _flat(S).copy(), sc.copy()
    kind, after = eng.estep_cert_info()["kind"], _totals(eng)
    eng.tune("estep_cert", 0)
    S0, sc0 = eng.estep(*canon)
    assert eng.estep_cert_info()["kind"] == "plain" and np.array_equal(_totals(eng), after)
    eng.tune("estep_cert", 1)
    assert np.array_equal(S, _flat(S0)) and np.array_equal(sc, sc0, equal_nan=True), kind
    assert np.isfinite(S).all() and np.isfinite(sc[0])
    return kind, after - before


@pytest.mark.parametrize("D,num_cu", [(14, 1), (16, 1), (16, 0)])
@pytest.mark.parametrize("case", [1, 2, 3, 4, 5])
def test_proven_waves_normalise_on_the_live_block(eng, case, D, num_cu):
    mus, W, ch = _params(K, D, 80.0, 5 + D)
    ref = _canonical(mus, W, ch)
    Z = _data(case, D, mus, ref)
    eng.tune("num_cu", num_cu)
    eng.upload(Z)
    eng.set_component_order(np.arange(K, dtype=np.int32))
    assert eng.plan(K)["kind"] == "fused" and eng.plan(K)["component_order"]
    assert (_both(eng, ref)[0], _both(eng, ref)[0]) == ("plain", "reference")

    # the first certified pass, nothing moved: the construction decides every row
    proven, one, all_wt, waves, need = _host_model(Z, ref, ref)
    expected = np.zeros((TILES, 4), dtype=bool)
    expected[AT[case], list(PROVEN_WAVES[case])] = True
    assert np.array_equal(waves, expected), waves
    assert proven == sum(not isinstance(r, tuple) for r in _layout(case, D))
    if case == 5:
        assert need[AT[5], 0] == 20                                   # its owner wave runs the two-group code
    kind, rose = _both(eng, ref)
    print("case %d: rows proven %d, one group %d of %d, proven waves %d" % (case, *rose))
    assert kind == "certified" and rose.tolist() == [proven, one, all_wt, int(waves.sum())], (rose, proven, one, all_wt, waves.sum())
    assert rose[3] > 0

    # case 6: the posterior has moved
    cur = _canonical(*_moved(mus, W, ch, 1, 7 + case))
    proven, one, all_wt, waves, _ = _host_model(Z, ref, cur)
    kind, rose = _both(eng, cur)
    print("        moved: rows proven %d, one group %d of %d, proven waves %d" % tuple(rose))
    assert kind == "certified" and rose.tolist() == [proven, one, all_wt, int(waves.sum())], (rose, proven, one, all_wt, waves.sum())
