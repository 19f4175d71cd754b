"""CPU: batched SVI without a GPU — the new entry point fails loudly on a null context, the rows= validation of
BatchedHipEngine.estep happens before any library call, and meanfield_stochastic_descent_batched on a duck-typed batched
engine backed by the CPU oracle reproduces the reference's SVI fixtures (B = 1, global streams) and solo
meanfield_stochastic_descent runs (B = 3, per-model streams), restores the caller's generator states and draws nothing
while it validates its arguments."""
import random

import numpy as np
import numpy.random as npr
import pytest

from conftest import load_golden, rel_err, nw_of, mnw_of
import model_checks as mc
from oracle_engine import OracleEngine
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_stochastic_descent_batched


def test_rows_entry_point_fails_loudly_on_a_null_context():
    lib = _lib.load()
    c, b, W = np.zeros((1, 1)), np.zeros((1, 1, 1)), np.ones((1, 1, 1, 1))
    rows, off = np.zeros(1, dtype=np.int64), np.array([0, 1], dtype=np.int64)
    S, sc = np.empty((1, 3)), np.empty((1, 3))
    assert lib.mimo_estep_batched_rows(None, c.ctypes.data, b.ctypes.data, W.ctypes.data, 1, rows.ctypes.data,
                                       off.ctypes.data, 0, S.ctypes.data, sc.ctypes.data) == _lib.E_INVALID
    assert lib.mimo_estep_batched_rows(None, None, None, None, 1, None, None, 0, None, None) == _lib.E_INVALID


def _offline(rows, D):
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D = None, len(rows), D
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_rows_argument_validation():
    eng = _offline([5, 3, 0], 2)
    K = 4
    c, b, W = np.zeros((3, K)), np.zeros((3, K, 2)), np.zeros((3, K, 2, 2))
    i64 = lambda *a: np.array(a, dtype=np.int64)
    good = [i64(4, 0, 0, 2, 1, 3, 4), i64(), i64()]
    bad = [good[:2],                                                    # one selection per problem
           good + [i64()],
           [i64(0).reshape(1, 1), i64(), i64()],                        # ndim != 1
           [np.int64(0), i64(), i64()],
           [np.array([0., 1.]), i64(), i64()],                          # not integers
           [np.array([True, False]), i64(), i64()],
           [i64(5), i64(), i64()],                                      # outside [0, N_b)
           [i64(0, -1), i64(), i64()],
           [i64(), i64(3), i64()],
           [i64(), i64(), i64(0)]]                                      # an empty problem admits no index
    for rows in bad:
        with pytest.raises(ValueError):
            eng.estep(c, b, W, rows=rows)
    with pytest.raises(ValueError):
        eng.estep(c, b, W, rows=good, keep_lse=True)
    # well-formed arguments pass the validation (and then need the library: the offline object has none)
    for rows in (good, [np.array([1, 1], dtype=np.int32), np.array([2], dtype=np.uint8), i64()]):
        with pytest.raises(AttributeError):
            eng.estep(c, b, W, rows=rows)
        with pytest.raises(AttributeError):
            eng.estep(c, b, W, rows=rows, stats=False, entropy_split=True)


class OracleBatch:
    """Duck-typed batched engine on the CPU oracle: upload, estep(..., rows=), weighted_stats, row_off.  A selection pass is
    the oracle's E-step on Z_b[rows_b]."""
    device = 0

    def __init__(self):
        self.uploads = self.passes = 0

    def upload(self, arrays):
        self.Zs = [np.ascontiguousarray(z, dtype=float) for z in arrays]
        self.row_off = np.concatenate([[0], np.cumsum([len(z) for z in self.Zs])]).astype(np.int64)
        self.uploads += 1

    def _on(self, Z):
        eng = OracleEngine()
        eng.upload(Z)
        return eng

    def estep(self, c, b, W, stats=True, keep_lse=False, entropy_split=False, rows=None):
        assert not keep_lse
        self.passes += 1
        out = [self._on(Z if rows is None else Z[np.asarray(rows[i])]).estep(c[i], b[i], W[i], stats=stats)
               for i, Z in enumerate(self.Zs)]
        return ([S for S, _ in out] if stats else None), np.stack([sc for _, sc in out])

    def weighted_stats(self, tables=None, K=None):
        assert all(t.shape[1] == len(Z) for t, Z in zip(tables, self.Zs))
        return [self._on(Z).weighted_stats(t) for t, Z in zip(tables, self.Zs)]


def _ilr_after_warmup(g, seeds=None):
    """The ILR fixture's model as check_ilr_svi brings it to its SVI run (scaling transform, seeded Gibbs warm-up)."""
    kind, ilr = mc.build_ilr(g, OracleEngine())
    ilr.init_transform(g["X"], g["Y"])
    if seeds is None:
        seeds = (int(g["seed"]) + 1, int(g["seed"]) + 2)
    npr.seed(seeds[0])
    random.seed(seeds[1])
    ilr.resample(g["X"], g["Y"], init_labels='random', maxiter=3, progress_bar=False)
    return ilr


def test_one_ilr_model_reproduces_the_reference_fixture():
    g = load_golden("ilr_svi_dx2_dy1_k8")
    ilr = _ilr_after_warmup(g)                          # leaves numpy / random where check_ilr_svi starts its SVI run
    eng = OracleBatch()
    vlbs = meanfield_stochastic_descent_batched([ilr], [(g["X"], g["Y"])], randomize=False, maxiter=int(g["iters"]),
                                                step_size=5e-1, batch_size=64, engine=eng)
    assert len(vlbs) == 1 and eng.uploads == 1 and eng.passes == 2 * int(g["iters"])
    assert rel_err(np.array(vlbs[0]), g["svi_vlb"]) < 1e-7
    for a, b in zip(ilr.models.posterior.params, mnw_of(g, "svi_mpost")):
        assert rel_err(a, b) < 1e-6


def _fresh_gmm(g):
    return mc.build_gmm(g, OracleEngine())[1]


def test_one_gmm_reproduces_the_reference_fixture():
    g = load_golden("drivers_d3_k5_dir")
    seed, iters = int(g["seed"]), int(g["iters"])
    m = _fresh_gmm(g)
    npr.seed(seed + 31)
    random.seed(seed + 32)
    vlbs = meanfield_stochastic_descent_batched([m], [g["X"]], randomize=True, maxiter=iters, step_size=5e-2, batch_size=64,
                                                engine=OracleBatch())
    assert rel_err(np.array(vlbs[0]), g["svi_vlb"]) < 1e-8
    for a, b in zip(m.components.posterior.params, nw_of(g, "svi_post")):
        assert rel_err(a, b) < 1e-7


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("randomize", [False, True])
def test_three_gmms_on_their_own_streams_equal_solo_runs(randomize):
    g = load_golden("drivers_d3_k5_dir")
    iters = int(g["iters"])
    rng = np.random.default_rng(5)
    data = [g["X"], g["X"][:150], g["X"] + 0.05 * rng.standard_normal(g["X"].shape)]
    nseeds, pseeds = [11, 12, 11], [21, 22, 23]
    kw = dict(randomize=randomize, maxiter=iters, step_size=5e-2, batch_size=64)
    models = [_fresh_gmm(g) for _ in data]
    npr.seed(99)
    random.seed(98)
    nstate, pstate = npr.get_state(), random.getstate()
    vlbs = meanfield_stochastic_descent_batched(models, data, numpy_seeds=nseeds, python_seeds=pseeds,
                                                engine=OracleBatch(), **kw)
    assert _same_state(npr.get_state(), nstate) and random.getstate() == pstate
    for m, X, ns, ps, v in zip(models, data, nseeds, pseeds, vlbs):
        s = _fresh_gmm(g)
        npr.seed(ns)
        random.seed(ps)
        vs = s.meanfield_stochastic_descent(X, progress_bar=False, **kw)
        assert len(v) == iters
        assert rel_err(np.array(v), np.array(vs)) < 1e-8
        for a, b in zip(m.components.posterior.params, s.components.posterior.params):
            assert rel_err(a, b) < 1e-7


def test_three_ilr_models_on_their_own_streams_equal_solo_runs():
    g = load_golden("ilr_svi_dx2_dy1_k8")
    iters = int(g["iters"])
    rng = np.random.default_rng(6)
    X, Y = g["X"], g["Y"]
    data = [(X, Y), (X[:200], Y[:200]), (X + 0.05 * rng.standard_normal(X.shape), Y)]
    nseeds, pseeds = [31, 32, 33], [41, 41, 43]
    kw = dict(randomize=False, maxiter=iters, step_size=5e-1, batch_size=64)

    def build():
        out = []
        for x, y in data:
            kind, ilr = mc.build_ilr(g, OracleEngine())
            ilr.init_transform(x, y)
            out.append(ilr)
        return out
    models, solos = build(), build()
    vlbs = meanfield_stochastic_descent_batched(models, data, numpy_seeds=nseeds, python_seeds=pseeds,
                                                engine=OracleBatch(), **kw)
    for m, s, (x, y), ns, ps, v in zip(models, solos, data, nseeds, pseeds, vlbs):
        npr.seed(ns)
        random.seed(ps)
        vs = s.meanfield_stochastic_descent(x, y, progress_bar=False, **kw)
        assert rel_err(np.array(v), np.array(vs)) < 1e-7
        for a, b in zip(m.models.posterior.params, s.models.posterior.params):
            assert rel_err(a, b) < 1e-6


def test_states_are_restored_when_a_model_raises():
    g = load_golden("drivers_d3_k5_dir")
    models = [_fresh_gmm(g) for _ in range(2)]
    data = [g["X"], g["X"][:40]]                          # batch_size > N_1: random.sample raises at model 1
    npr.seed(7)
    random.seed(8)
    nstate, pstate = npr.get_state(), random.getstate()
    with pytest.raises(ValueError, match="[Ss]ample larger than population"):
        meanfield_stochastic_descent_batched(models, data, maxiter=3, batch_size=64, numpy_seeds=[1, 2],
                                             python_seeds=[3, 4], engine=OracleBatch())
    assert _same_state(npr.get_state(), nstate) and random.getstate() == pstate

    class Broken(OracleBatch):
        def estep(self, *a, **kw):
            if kw.get("rows") is not None:
                raise RuntimeError("pass failed")
            return super().estep(*a, **kw)
    with pytest.raises(RuntimeError):
        meanfield_stochastic_descent_batched(models, [g["X"], g["X"]], randomize=False, maxiter=3, batch_size=64,
                                             numpy_seeds=[1, 2], python_seeds=[3, 4], engine=Broken())
    assert _same_state(npr.get_state(), nstate) and random.getstate() == pstate


def test_argument_validation_draws_nothing():
    g = load_golden("drivers_d3_k5_dir")
    models = [_fresh_gmm(g) for _ in range(2)]
    data = [g["X"], g["X"][:100]]
    ilr = mc.build_ilr(load_golden("ilr_svi_dx2_dy1_k8"), OracleEngine())[1]
    nstate, pstate = npr.get_state(), random.getstate()
    eng = OracleBatch()
    for kw in (dict(numpy_seeds=[1]), dict(numpy_seeds=[1, 2, 3]), dict(python_seeds=[1]), dict(python_seeds=[1, 2, 3]),
               dict(batch_size=0)):
        with pytest.raises(ValueError):
            meanfield_stochastic_descent_batched(models, data, engine=eng, **kw)
    with pytest.raises(ValueError):
        meanfield_stochastic_descent_batched(models, data[:1], engine=eng)
    with pytest.raises(ValueError):
        meanfield_stochastic_descent_batched([], [], engine=eng)
    with pytest.raises(ValueError):
        meanfield_stochastic_descent_batched([models[0], ilr], data, engine=eng)
    assert eng.uploads == 0
    assert _same_state(npr.get_state(), nstate) and random.getstate() == pstate
