"""mimo_set_component_order: the fused mean-field pass with component order[s] in slot s.  Whatever the order, the caller sees
its own numbering: statistics and scalars match the oracle as they do in the identity, the skipping and the dense pass keep
bit-equal scalars, repeats and the asynchronous call return the same bits, and a cleared order leaves the bits of a context
that never had one.  The posteriors have pairs of overlapping components which the identity puts into different row blocks;
the shapes reach the skipping instantiation with four full row blocks (Dz = 16, K = 64), three row blocks with padding slots
(Dz = 14, K = 40) and the split instantiation of K <= 32 (Dz = 16, K = 17), with two and four tiles and a ragged last one."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import mimo_oracle as O
from mimo_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64), (14, 40), (16, 17)]
ROWS = [33, 97]
ORDERS = ["identity", "random", "rotation", "block_order"]


def _problem(D, K, N):
    """W = I, means 40 apart; every third component shares its mean (up to 0.3) with the one 16 further on, i.e. in the next
    row block; rows drawn around the means of all components."""
    rng = np.random.default_rng(100 * D + K + N)
    k = np.arange(K)
    mus = np.zeros((K, D))
    mus[k, k % D] = 40.0 * (1 + k // D)
    for a in range(0, K - 16, 3):
        mus[a + 16] = mus[a] + 0.3 * rng.standard_normal(D)
    W = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    b = mus.copy()
    c = -0.5 * np.einsum("ki,ki->k", b, mus) + rng.standard_normal(K) * 0.1
    comp = rng.integers(K, size=N)
    Z = np.ascontiguousarray(mus[comp] + rng.standard_normal((N, D)))
    return Z, c, b, W, mus, np.bincount(comp, minlength=K) + 2.0        # (mass: no component is a filler)


_REF = {}


def _reference(D, K, N):
    """oracle statistics and scalars, once per shape"""
    if (D, K, N) not in _REF:
        Z, c, b, W, _, _ = _problem(D, K, N)
        L = O.canonical_eval(Z, c, b, W)
        lse = logsumexp(L, axis=0)
        n, sx, sxx = O.packed_stats(Z, np.exp(L - lse))
        _REF[(D, K, N)] = (np.concatenate([np.ravel(n), np.ravel(sx), np.ravel(sxx)]), float(lse.sum()))
    return _REF[(D, K, N)]


def _order(kind, K, mus, mass):
    if kind == "identity":
        return np.arange(K, dtype=np.int32)
    if kind == "random":
        return np.random.default_rng(K).permutation(K).astype(np.int32)
    if kind == "rotation":
        return np.roll(np.arange(K, dtype=np.int32), -16)          # slot s holds component s + 16: every block moves on by one
    order = np.empty(K, dtype=np.int32)
    means = np.ascontiguousarray(mus)
    assert _lib.load().mimo_host_block_order(K, mus.shape[1], means.ctypes.data, mass.ctypes.data, 16, order.ctypes.data) == 0
    return order


def _flat(S):
    return np.concatenate([S.n.ravel(), S.sx.ravel(), S.sxx.ravel()])


def _pass(engine, v, c, b, W):
    engine.tune("resp_skip_log2", v)
    S, sc = engine.estep(c, b, W)
    return _flat(S), sc.copy()


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.fixture(scope="module")
def fresh():
    """a context no order is ever set on"""
    from mimo_amd.engine import HipEngine
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.fixture
def ordered_engine(engine):
    engine.tune("mid_min_d", 64)                                   # K <= 48 at these Dz would otherwise take the mid kernel (ROUTING.md)
    yield engine
    engine.tune("resp_skip_log2", 60)
    engine.tune("block_order", 1)
    engine.tune("mid_min_d", 0)
    engine.set_component_order(None)


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("D,K", SHAPES)
def test_pass_under_an_order(ordered_engine, fresh, D, K, N, kind):
    engine = ordered_engine
    Z, c, b, W, mus, mass = _problem(D, K, N)
    ref, ref_lse = _reference(D, K, N)
    order = _order(kind, K, mus, mass)
    assert sorted(order) == list(range(K))
    if kind == "block_order":                                      # the pairs the identity splits share a block now
        blk = np.empty(K, dtype=int)
        blk[order] = np.arange(K) // 16
        pairs = [(a, a + 16) for a in range(0, K - 16, 3) if mass[a] >= 1 and mass[a + 16] >= 1]
        assert pairs and all(blk[a] == blk[a2] for a, a2 in pairs)
    engine.upload(Z)
    assert engine.plan(K)["kind"] == "fused" and not engine.plan(K)["component_order"]
    engine.set_component_order(order)
    assert engine.plan(K)["component_order"]
    skip, sc_skip = _pass(engine, 60, c, b, W)
    skip2, sc_skip2 = _pass(engine, 60, c, b, W)
    dense, sc_dense = _pass(engine, 0, c, b, W)
    engine.tune("resp_skip_log2", 60)
    engine.estep_async(c, b, W)
    S_a, sc_a = engine.estep_wait()
    print("order %s Dz=%d K=%d N=%d: skip vs oracle %.2e, skip vs dense %.2e, lse %.2e"
          % (kind, D, K, N, _rel(skip, ref), _rel(skip, dense), abs(sc_skip[0] - ref_lse) / abs(ref_lse)))
    assert _rel(skip, ref) < 1e-11
    assert abs(sc_skip[0] - ref_lse) < 1e-11 * abs(ref_lse)
    assert _rel(skip, dense) < 1e-13
    assert np.array_equal(sc_skip, sc_dense, equal_nan=True)
    assert np.array_equal(skip, skip2) and np.array_equal(sc_skip, sc_skip2, equal_nan=True)
    assert np.array_equal(_flat(S_a), skip) and np.array_equal(sc_a, sc_skip, equal_nan=True)
    # cleared: the bits of a context that never had an order
    engine.set_component_order(None)
    assert not engine.plan(K)["component_order"]
    fresh.upload(Z)                                                # ("mid_min_d" is process-wide: it holds here too)
    try:
        for v in (60, 0):
            got, want = _pass(engine, v, c, b, W), _pass(fresh, v, c, b, W)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    finally:
        fresh.tune("resp_skip_log2", 60)


def test_an_order_is_dropped_with_its_shape(ordered_engine):
    """Another K, a new data set, the tuning key: each leaves the identity behind."""
    engine = ordered_engine
    D, K, N = 16, 64, 97
    Z, c, b, W, _, _ = _problem(D, K, N)
    order = _order("random", K, None, None)
    engine.upload(Z)
    engine.set_component_order(order)
    assert engine.plan(K)["component_order"]
    engine.upload(Z)
    assert not engine.plan(K)["component_order"]
    engine.set_component_order(order)
    engine.estep(c[:48], b[:48], W[:48])
    assert not engine.plan(K)["component_order"]
    engine.set_component_order(order)
    engine.tune("block_order", 0)
    assert not engine.plan(K)["component_order"]
    engine.set_component_order(order)                              # a no-op now
    assert not engine.plan(K)["component_order"]
    engine.tune("block_order", 1)
    engine.set_component_order(order)
    assert engine.plan(K)["component_order"]


def test_a_non_permutation_is_refused(ordered_engine):
    engine = ordered_engine
    D, K, N = 16, 64, 97
    Z, c, b, W, _, _ = _problem(D, K, N)
    order = _order("random", K, None, None)
    engine.upload(Z)
    engine.set_component_order(order)
    before = _pass(engine, 60, c, b, W)
    lib, ctx = engine._lib, engine._ctx

    def refused(bad, n, text):
        bad = np.ascontiguousarray(bad, dtype=np.int32)
        rc = lib.mimo_set_component_order(ctx, bad.ctypes.data, n)
        assert rc == _lib.E_INVALID, (rc, lib.mimo_last_error(ctx).decode())
        assert lib.mimo_last_error(ctx).decode() == text

    twice = order.copy()
    twice[5] = twice[2]
    refused(twice, K, "mimo_set_component_order: component %d sits in two slots (the second: 5)" % twice[2])
    high = order.copy()
    high[7] = K
    refused(high, K, "mimo_set_component_order: order[7] = 64 is no component of 0 .. 63")
    low = order.copy()
    low[0] = -1
    refused(low, K, "mimo_set_component_order: order[0] = -1 is no component of 0 .. 63")
    refused(order, 0, "mimo_set_component_order: K = 0 outside [1, 256]")
    refused(order, 257, "mimo_set_component_order: K = 257 outside [1, 256]")
    with pytest.raises(ValueError):
        engine.set_component_order(twice)
    # the order set before them is still in force
    assert engine.plan(K)["component_order"]
    after = _pass(engine, 60, c, b, W)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)


def test_routes_outside_the_scope_ignore_the_order(ordered_engine):
    """A label pass and a softmax pass that keeps the responsibility table: the same bits with and without an order."""
    engine = ordered_engine
    D, K, N = 16, 64, 97
    Z, c, b, W, _, _ = _problem(D, K, N)
    order = _order("random", K, None, None)
    engine.upload(Z)

    def run():
        labels, S_g = engine.gibbs_labels(c, b, W, seed=3, sweep=1)
        S_r, sc_r = engine.estep(c, b, W, keep_resp=True)
        resp = engine.get_resp(K).copy()
        _, sc_b = engine.estep(c, b, W, stats=False)
        return labels, _flat(S_g), _flat(S_r), sc_r.copy(), resp, sc_b.copy()

    plain = run()
    engine.set_component_order(order)
    ordered = run()
    for x, y in zip(plain, ordered):
        assert np.array_equal(x, y, equal_nan=True)


def test_device_block_in_the_callers_numbering(ordered_engine):
    """The device block a sharded engine all-reduces (MIMO_F_DEVICE_OUT): the rows of the caller's components, and the bits of
    the host delivery under the same order."""
    import torch
    engine = ordered_engine
    D, K, N = 16, 64, 97
    Z, c, b, W, mus, mass = _problem(D, K, N)
    ref, ref_lse = _reference(D, K, N)
    order = _order("block_order", K, mus, mass)
    engine.upload(Z)
    engine.set_component_order(order)
    host, sc_host = _pass(engine, 60, c, b, W)
    slen = K * (1 + D + D * D)
    buf = torch.zeros(slen + 4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    engine.estep_device(c, b, W, buf.data_ptr(), buf.data_ptr() + 8 * slen)
    engine.set_stream(0)                                           # (synchronises the context's stream)
    out = buf.cpu().numpy()
    from mimo_amd.engine import SuffStats
    dev = _flat(SuffStats.from_packed(out[:slen], K, D))
    assert np.array_equal(dev, host) and np.array_equal(out[slen:slen + 3], sc_host, equal_nan=True)
    assert _rel(dev, ref) < 1e-11


def test_tuning_a_context_knob_leaves_the_router_alone(ordered_engine):
    """mimo_tune writes the knob of its key and nothing else: Dz = 1, K = 200 runs on the narrow kernels of mimo_narrow_big.hip only
    while the process-wide "narrow_big_vi" stands at its default, so a key that leaked into it would move this shape elsewhere."""
    engine = ordered_engine
    engine.tune("mid_min_d", 0)
    rng = np.random.default_rng(3)
    engine.upload(rng.standard_normal((500, 1)))
    assert engine.plan(200)["kind"] == "narrow"
    for key, values in (("block_order", (1, 0, 1)), ("resp_skip_log2", (60, 0, 60)), ("mid_min_d", (64, 0)), ("mid_narrow_k", (40, 0)),
                        ("mid_labels_min_d", (20, 0)), ("mid_labels_narrow_k", (8, 0)), ("num_cu", (3, 0)), ("sorted_range", (5, 0))):
        for v in values:
            engine.tune(key, v)
            assert engine.plan(200)["kind"] == "narrow", (key, v)
    engine.tune("narrow_big_vi", 160)                              # the key itself still works
    assert engine.plan(200)["kind"] != "narrow"
    engine.tune("narrow_big_vi", 0)
    assert engine.plan(200)["kind"] == "narrow"


def test_all_reduced_block_in_the_callers_numbering():
    """A context with the library's own communicator (one rank): the block is unpacked on the device, all-reduced there and then
    copied, not written straight to pinned memory.  Under an order it must deliver the bits of the context without one."""
    from mimo_amd.engine import HipEngine
    D, K, N = 16, 64, 97
    Z, c, b, W, mus, mass = _problem(D, K, N)
    ref, _ = _reference(D, K, N)
    eng = HipEngine(0)
    try:
        eng.upload(Z)
        for kind in ("block_order", "random"):
            order = _order(kind, K, mus, mass)
            eng.set_component_order(order)
            S0, sc0 = eng.estep(c, b, W)
            eng.comm_init(HipEngine.comm_unique_id(), 0, 1)
            eng.set_component_order(order)
            assert eng.plan(K)["component_order"]
            S1, sc1 = eng.estep(c, b, W)
            eng.estep_async(c, b, W)
            S2, sc2 = eng.estep_wait()
            eng.comm_destroy()
            assert np.array_equal(_flat(S1), _flat(S0)) and sc1[0] == sc0[0]
            assert np.array_equal(_flat(S2), _flat(S0)) and sc2[0] == sc0[0]
            assert _rel(_flat(S1), ref) < 1e-11
    finally:
        eng.close()
