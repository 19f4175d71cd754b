"""Where an input comes from and where a result goes must not change a bit of it.  Every entry point that takes a table, labels,
weights or uniforms reads them from the context's resident copy (NULL), from host memory (staged by the library) or from device
memory (MIMO_F_DEVICE_IN); every pass hands its packed block out synchronously, through mimo_wait or into device memory.  The same
kernel reads the same values each way, so all comparisons are exact.  Also here: buffers that grow and are reused over a sequence
of calls of different shapes, and a context that goes from a batch to single data and back."""
import ctypes as C

import numpy as np
import pytest

from mimo_amd import _lib
from mimo_amd.engine import _ptr

pytestmark = pytest.mark.gpu

N = 1027                      # four full 256-row tiles and three rows; no multiple of 64
D0, K0 = 3, 5
TWO_STAGE = (32, 128)         # the pass keeps its (K, N) table in the context's own resp buffer there
NAN_ROWS = (0, 511, 1026)
F = _lib
SEED, SWEEP = 5, 2


def _model(rng, K, D, diag=False, lead=()):
    A = rng.standard_normal(lead + (K, D, D))
    W = A @ np.swapaxes(A, -1, -2) / D + 0.3 * np.eye(D)
    if diag:
        W = W * np.eye(D)
    return rng.standard_normal(lead + (K,)), rng.standard_normal(lead + (K, D)), np.ascontiguousarray(W)


def _case(name):
    """(rows, c, b, W, K) of a named case; the same values every time it is asked for."""
    D, K = TWO_STAGE if name == "two-stage" else (D0, K0)
    rng = np.random.default_rng(1000 * D + K)
    Z = rng.standard_normal((N, D)) * 1.5
    if name == "nan":
        Z[list(NAN_ROWS), 1] = np.nan
    return (np.ascontiguousarray(Z),) + _model(rng, K, D) + (K,)


class _Ctx:
    """A HipEngine's context, driven through ctypes."""

    def __init__(self, Z=None):
        from mimo_amd.engine import HipEngine
        self.eng = HipEngine(0)
        self.lib, self.ctx = self.eng._lib, self.eng._ctx
        if Z is not None:
            self.upload(Z)

    def ok(self, rc):
        assert rc == 0, (rc, self.error())

    def error(self):
        return self.lib.mimo_last_error(self.ctx).decode()

    def upload(self, Z):
        self.N, self.D = Z.shape
        self.ok(self.lib.mimo_upload(self.ctx, _ptr(Z), self.N, self.D))

    def slen(self, K):
        return K * (1 + self.D + self.D * self.D)

    def estep(self, c, b, W, K, flags=0):
        S, sc = np.full(self.slen(K), np.nan), np.full(3, np.nan)
        self.ok(self.lib.mimo_estep(self.ctx, _ptr(c), _ptr(b), _ptr(W), K, flags, _ptr(S), _ptr(sc)))
        return S, sc

    def gibbs(self, c, b, W, K, u=None, flags=0):
        S, labels = np.full(self.slen(K), np.nan), np.full(self.N, -7, dtype=np.int32)
        self.ok(self.lib.mimo_gibbs_labels(self.ctx, _ptr(c), _ptr(b), _ptr(W), K, SEED, SWEEP, u, flags, _ptr(labels), _ptr(S)))
        return labels, S

    def table(self, getter, K):
        out = np.full((K, self.N), np.nan)
        self.ok(getter(self.ctx, _ptr(out)))
        return out

    def close(self):
        self.eng.close()


def _dev(a):
    """The array on the GPU, complete before anyone else's stream reads it (the library runs on its own non-blocking stream)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _all_equal(results):
    first = results[0]
    for r in results[1:]:
        for x, y in zip(first, r):
            assert np.array_equal(x, y, equal_nan=True)


def test_two_stage_shape_is_two_stage():
    out = (C.c_int64 * 8)()
    assert _lib.load().mimo_plan_shape(TWO_STAGE[0], TWO_STAGE[1], 0, N, 0, out, None, 0) == 0
    assert out[0] == 2        # MIMO_PLAN_TWO_STAGE


@pytest.mark.parametrize("name", ["default", "nan"])
def test_weighted_stats_sources(name):
    Z, c, b, W, K = _case(name)
    x = _Ctx(Z)
    x.estep(c, b, W, K, F.F_KEEP_RESP)
    R = x.table(x.lib.mimo_get_resp, K)
    Rd = _dev(R)
    got = []
    for src, flags in ((None, 0), (_ptr(R), 0), (Rd.data_ptr(), F.F_DEVICE_IN)):
        S = np.full(x.slen(K), np.nan)
        x.ok(x.lib.mimo_weighted_stats(x.ctx, src, K, flags, _ptr(S)))
        got.append((S,))
    _all_equal(got)
    assert np.isfinite(got[0][0]).all()
    x.close()


@pytest.mark.parametrize("name", ["default", "nan", "two-stage"])
def test_label_stats_sources(name):
    Z, c, b, W, K = _case(name)
    x = _Ctx(Z)
    L, _ = x.gibbs(c, b, W, K)
    assert L.min() >= 0 and L.max() < K
    Ld = _dev(L)
    got = []
    for src, flags in ((None, 0), (_ptr(L), 0), (Ld.data_ptr(), F.F_DEVICE_IN)):
        S = np.full(x.slen(K), np.nan)
        x.ok(x.lib.mimo_label_stats(x.ctx, src, K, flags, _ptr(S)))
        got.append((S,))
    _all_equal(got)
    assert got[0][0].reshape(K, -1)[:, 0].sum() == N - (len(NAN_ROWS) if name == "nan" else 0)
    x.close()


@pytest.mark.parametrize("name", ["default", "nan", "two-stage"])
def test_gibbs_uniform_sources(name):
    Z, c, b, W, K = _case(name)
    x = _Ctx(Z)
    u = np.random.default_rng(9).random(N)
    ud = _dev(u)
    _all_equal([x.gibbs(c, b, W, K, _ptr(u)), x.gibbs(c, b, W, K, ud.data_ptr(), F.F_DEVICE_IN)])
    x.close()


@pytest.mark.parametrize("name", ["default", "nan"])
def test_weighted_estep_sources(name):
    Z, c, b, W, K = _case(name)
    x = _Ctx(Z)
    w = np.random.default_rng(10).random(N) + 0.25
    wd = _dev(w)

    def run(src, flags):
        S, sc = np.full(x.slen(K), np.nan), np.full(3, np.nan)
        rc = x.lib.mimo_estep_weighted(x.ctx, _ptr(c), _ptr(b), _ptr(W), K, src, flags, _ptr(S), _ptr(sc))
        return rc, (S, sc)

    results = []
    for src, flags in ((_ptr(w), 0), (None, F.F_WEIGHTS_RESIDENT), (wd.data_ptr(), F.F_DEVICE_IN)):
        rc, r = run(src, flags)
        x.ok(rc)
        results.append(r)
    _all_equal(results)
    # uniforms of a label pass take the buffer the weights were resident in
    x.gibbs(c, b, W, K, _ptr(w / 2))
    rc, _ = run(None, F.F_WEIGHTS_RESIDENT)
    assert rc == F.E_STATE and x.error() == "mimo_estep_weighted: no row weights are resident on the device"
    x.close()


def test_weighted_estep_refuses_the_two_stage_shape():
    Z, c, b, W, K = _case("two-stage")
    x = _Ctx(Z)
    w, S, sc = np.ones(N), np.empty(x.slen(K)), np.empty(3)
    rc = x.lib.mimo_estep_weighted(x.ctx, _ptr(c), _ptr(b), _ptr(W), K, _ptr(w), 0, _ptr(S), _ptr(sc))
    assert rc == F.E_UNSUPPORTED
    assert x.error() == (f"mimo_estep_weighted: K={K}, Dz={TWO_STAGE[0]} runs on the two-stage path, which takes "
                         "its weights as a table (mimo_estep + mimo_weighted_stats)")
    x.close()


@pytest.mark.parametrize("name", ["default", "nan", "two-stage"])
def test_sample_from_log_sources(name):
    """MIMO_F_DEVICE_IN speaks for the table and the uniforms together, so a host table goes with host uniforms and a device table
    with device uniforms; the resident table and the Philox draw (u NULL) go with either."""
    Z, c, b, W, K = _case(name)
    x = _Ctx(Z)
    x.estep(c, b, W, K, F.F_KEEP_LOGP)
    T = x.table(x.lib.mimo_get_logp, K)
    u = np.random.default_rng(11).random(N)
    Td, ud = _dev(T), _dev(u)

    def draw(table, uni, flags):
        labels, ln = np.full(N, -7, dtype=np.int32), np.full(N, np.nan)
        x.ok(x.lib.mimo_sample_from_log(x.ctx, table, K, N, uni, SEED, SWEEP, flags, _ptr(labels), _ptr(ln)))
        return labels, ln

    given = [draw(None, _ptr(u), 0), draw(None, ud.data_ptr(), F.F_DEVICE_IN), draw(_ptr(T), _ptr(u), 0),
             draw(Td.data_ptr(), ud.data_ptr(), F.F_DEVICE_IN)]
    _all_equal(given)
    philox = [draw(None, None, 0), draw(_ptr(T), None, 0), draw(Td.data_ptr(), None, F.F_DEVICE_IN)]
    _all_equal(philox)
    for labels, ln in (given[0], philox[0]):
        assert labels.min() >= 0 and labels.max() < K and np.isfinite(ln).all()
    x.close()


@pytest.mark.parametrize("name", ["default", "nan"])
def test_table_entropy_sources(name):
    Z, c, b, W, K = _case(name)
    x = _Ctx(Z)
    x.estep(c, b, W, K, F.F_KEEP_RESP)
    R = x.table(x.lib.mimo_get_resp, K)
    Rd = _dev(R)
    got = []
    for src, count, flags in ((None, 0, 0), (_ptr(R), K * N, 0), (Rd.data_ptr(), K * N, F.F_DEVICE_IN)):
        out = C.c_double(np.nan)
        x.ok(x.lib.mimo_table_entropy(x.ctx, src, count, flags, C.byref(out)))
        got.append((np.array(out.value),))
    _all_equal(got)
    assert np.isfinite(got[0][0])
    x.close()


@pytest.mark.parametrize("D,K", [(D0, K0), (8, 40)])
@pytest.mark.parametrize("structure", [0, 1], ids=["full", "diag"])
def test_deliveries_agree(structure, D, K):
    """Synchronous, MIMO_F_ASYNC + mimo_wait, and MIMO_F_DEVICE_OUT.  The full structure's block is reduced straight into pinned
    host memory, the diagonal structure's goes through the device block and a copy."""
    import torch
    rng = np.random.default_rng(100 * D + K + structure)
    Z = rng.standard_normal((N, D)) * 1.5
    c, b, W = _model(rng, K, D, diag=structure == 1)
    x = _Ctx(Z)
    x.ok(x.lib.mimo_set_structure(x.ctx, structure))
    sync = x.estep(c, b, W, K)
    S, sc = np.full(x.slen(K), np.nan), np.full(3, np.nan)
    x.ok(x.lib.mimo_estep(x.ctx, _ptr(c), _ptr(b), _ptr(W), K, F.F_ASYNC, None, None))
    x.ok(x.lib.mimo_wait(x.ctx, _ptr(S), _ptr(sc)))
    Sd = torch.full((x.slen(K),), float("nan"), dtype=torch.float64, device="cuda")
    scd = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    x.ok(x.lib.mimo_estep(x.ctx, _ptr(c), _ptr(b), _ptr(W), K, F.F_DEVICE_OUT, Sd.data_ptr(), scd.data_ptr()))
    again = x.estep(c, b, W, K)          # (a synchronous call on the same stream: the pass before it is done)
    _all_equal([sync, (S, sc), (Sd.cpu().numpy(), scd.cpu().numpy()), again])
    assert np.isfinite(sync[0]).all() and np.isfinite(sync[1][0])
    x.close()


def test_wait_refuses_statistics_nobody_computed():
    Z, c, b, W, K = _case("default")
    x = _Ctx(Z)
    S, sc = np.empty(x.slen(K)), np.empty(3)
    x.ok(x.lib.mimo_estep(x.ctx, _ptr(c), _ptr(b), _ptr(W), K, F.F_NO_STATS | F.F_ASYNC, None, None))
    assert x.lib.mimo_wait(x.ctx, _ptr(S), _ptr(sc)) == F.E_STATE
    assert x.error() == "mimo_wait: the pending call produced no statistics"
    x.close()


def test_buffers_are_reused_over_a_sequence_of_shapes():
    """One context through growing and shrinking K and N; every call equals the same call on a fresh context."""
    rng = np.random.default_rng(12)
    Z = rng.standard_normal((5003, D0)) * 1.5
    small, big = _model(rng, 5, D0), _model(rng, 40, D0)
    keep = F.F_KEEP_RESP | F.F_KEEP_LOGP | F.F_KEEP_LSE
    steps = [(1027, lambda x: x.estep(*small, 5)), (None, lambda x: x.estep(*big, 40, keep)), (None, lambda x: x.estep(*small, 5)),
             (300, lambda x: x.estep(*big, 40)), (5003, lambda x: x.gibbs(*small, 5))]
    x, rows = _Ctx(), None
    for n, call in steps:
        if n is not None:
            rows = np.ascontiguousarray(Z[:n])
            x.upload(rows)
        fresh = _Ctx(rows)
        _all_equal([call(x), call(fresh)])
        fresh.close()
    x.close()


def _upload_batched(x, rng, rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum(rows)
    Z = np.ascontiguousarray(rng.standard_normal((int(off[-1]), D0)) * 1.5)
    x.ok(x.lib.mimo_upload_batched(x.ctx, _ptr(Z), _ptr(off), len(rows), D0))
    x.D = D0
    c, b, W = _model(rng, K0, D0, lead=(len(rows),))
    S, sc = np.full((len(rows), x.slen(K0)), np.nan), np.full((len(rows), 3), np.nan)
    x.ok(x.lib.mimo_estep_batched(x.ctx, _ptr(c), _ptr(b), _ptr(W), K0, 0, _ptr(S), _ptr(sc)))
    assert np.isfinite(S).all() and np.isfinite(sc[:, 0]).all()
    return S


def test_a_batch_then_single_data_then_a_batch():
    rng = np.random.default_rng(13)
    x = _Ctx()
    S = _upload_batched(x, rng, [100, 0, 227])
    assert [round(S[p].reshape(K0, -1)[:, 0].sum()) for p in range(3)] == [100, 0, 227]
    Z, c, b, W, K = _case("default")
    x.upload(Z)
    fresh = _Ctx(Z)
    _all_equal([x.estep(c, b, W, K), fresh.estep(c, b, W, K)])
    fresh.close()
    _upload_batched(x, rng, [64, 300, 1, 257, 5])
    assert x.lib.mimo_destroy(x.ctx) == 0
    x.eng._ctx = None
