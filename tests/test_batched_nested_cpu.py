"""CPU: the nested batch without a GPU — the header declares the four entry points and each fails loudly on a null
context, the row_weights= / log_gating / upload_shared validation of BatchedHipEngine happens before any library call, and
meanfield_coordinate_descent_nested on a duck-typed shared batch backed by the CPU oracle reproduces the reference's
mixture-of-mixtures fixtures and the solo driver's run from the same seeds."""
import os
import re

import numpy as np
import numpy.random as npr
import pytest
from scipy.special import logsumexp

from conftest import ROOT, load_golden, rel_err
from oracle_engine import OracleEngine
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import expected_responsibilities_nested, meanfield_coordinate_descent_nested

NAMES = ("mimo_upload_batched_shared", "mimo_estep_batched_weighted", "mimo_outer_resp_batched",
         "mimo_get_row_weights_batched")
FIXTURES = ("hier_gmm_d2_k4_m2", "hier_gmm_d3_k3_m3")


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES


def test_entry_points_fail_loudly_on_a_null_context():
    lib = _lib.load()
    z, out = np.zeros((1, 1)), np.empty(4)
    c, b, W = np.zeros((1, 1)), np.zeros((1, 1, 1)), np.ones((1, 1, 1, 1))
    assert lib.mimo_upload_batched_shared(None, z.ctypes.data, 1, 1, 1) == _lib.E_INVALID
    assert lib.mimo_estep_batched_weighted(None, c.ctypes.data, b.ctypes.data, W.ctypes.data, 1, z.ctypes.data, 0,
                                           out.ctypes.data, out.ctypes.data) == _lib.E_INVALID
    assert lib.mimo_outer_resp_batched(None, z.ctypes.data, 0, out.ctypes.data) == _lib.E_INVALID
    assert lib.mimo_get_row_weights_batched(None, out.ctypes.data) == _lib.E_INVALID


def _offline(rows, D, shared=False):
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D, eng.shared = None, len(rows), D, shared
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_row_weights_argument_validation():
    K = 3
    c, b, W = np.zeros((2, K)), np.zeros((2, K, 2)), np.zeros((2, K, 2, 2))
    ragged, shared = _offline([5, 3], 2), _offline([4, 4], 2, shared=True)
    bad_ragged = [[np.ones(5)],                                        # one vector per problem
                  [np.ones(5), np.ones(3), np.ones(1)],
                  [np.ones(4), np.ones(3)],                             # one weight per datum
                  [np.ones(5), np.ones(4)],
                  [np.ones(5), np.array([1., -1e-300, 1.])],            # negative
                  [np.ones(5), np.array([1., np.nan, 1.])],             # not finite
                  [np.array([np.inf, 1., 1., 1., 1.]), np.ones(3)],
                  np.ones((2, 4)),                                      # a (B, N) array needs a shared batch
                  'device', '']
    for w in bad_ragged:
        with pytest.raises(ValueError):
            ragged.estep(c, b, W, row_weights=w)
    bad_shared = [np.ones((2, 5)), np.ones((3, 4)), np.ones((1, 8)), -np.ones((2, 4)), np.full((2, 4), np.nan),
                  [np.ones(4), np.ones(3)]]
    for w in bad_shared:
        with pytest.raises(ValueError):
            shared.estep(c, b, W, row_weights=w)
    # not together with a row selection, whatever the weights are
    sel = [np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)]
    for w in ([np.ones(5), np.ones(3)], 'resident'):
        with pytest.raises(ValueError):
            ragged.estep(c, b, W, rows=sel, row_weights=w)
    # well-formed arguments pass the validation (and then need the library: the offline object has none)
    for eng, w in ((ragged, [np.ones(5), np.zeros(3)]), (ragged, [np.ones((1, 5)), np.ones(3)]), (ragged, 'resident'),
                   (shared, np.ones((2, 4))), (shared, [np.ones(4), np.zeros(4)]), (shared, 'resident')):
        with pytest.raises(AttributeError):
            eng.estep(c, b, W, row_weights=w)
        with pytest.raises(AttributeError):
            eng.estep(c, b, W, row_weights=w, keep_lse=True, entropy_split=True)


def test_upload_shared_and_log_gating_validation():
    eng = _offline([4, 4], 2, shared=True)
    for Z, B in ((np.zeros((0, 2)), 2), (np.zeros(4), 2), (np.zeros((4, 2, 1)), 2), (np.zeros((4, 2)), 0),
                 (np.zeros((4, 2)), -1)):
        with pytest.raises(ValueError):
            eng.upload_shared(Z, B)
    assert eng.B == 2 and eng.shared                       # a refused upload leaves the object as it was
    for lg in (np.zeros(3), np.zeros(1), np.array([0., np.nan]), np.array([np.inf, 0.]), np.array([-np.inf, -np.inf])):
        with pytest.raises(ValueError):
            eng.outer_responsibilities(lg)
    for call in (lambda: eng.upload_shared(np.zeros((4, 2)), 2), lambda: eng.outer_responsibilities(np.array([0., -np.inf])),
                 eng.get_row_weights):
        with pytest.raises(AttributeError):
            call()


class OracleNested:
    """Duck-typed shared batch on the CPU oracle: what meanfield_coordinate_descent_nested uses of BatchedHipEngine."""
    device = 0

    def __init__(self):
        self.uploads = self.table_uploads = 0
        self.w = self.lse = None

    def set_structure(self, structure):
        assert structure == 'full'

    def upload_shared(self, Z, B):
        self.eng = OracleEngine()
        self.eng.upload(Z)
        self.B, N = int(B), len(Z)
        self.row_off = np.arange(self.B + 1, dtype=np.int64) * N
        self.uploads += 1
        self.w = self.lse = None

    def estep(self, c, b, W, stats=True, keep_lse=False, entropy_split=False, rows=None, row_weights=None):
        assert rows is None and c.shape[0] == self.B
        if isinstance(row_weights, str):
            assert row_weights == 'resident' and self.w is not None
        elif row_weights is not None:
            self.w = np.array(row_weights, dtype=float).reshape(self.B, -1)
            self.table_uploads += 1
        out, lse = [], []
        for i in range(self.B):
            out.append(self.eng.estep(c[i], b[i], W[i], stats=stats, keep_lse=True,
                                      row_weights=None if row_weights is None else self.w[i]))
            lse.append(self.eng.get_lse())
        self.lse = np.stack(lse) if keep_lse else None
        return ([S for S, _ in out] if stats else None), np.stack([sc for _, sc in out])

    def weighted_stats(self, tables=None, K=None):
        assert len(tables) == self.B
        return [self.eng.weighted_stats(t) for t in tables]

    def outer_responsibilities(self, log_gating):
        assert self.lse is not None
        t = self.lse + np.asarray(log_gating, dtype=float)[:, None]
        l = logsumexp(t, axis=0)
        self.w = np.exp(t - l)
        return self.w.sum(axis=1), float(l.sum())

    def get_row_weights(self):
        return [w.copy() for w in self.w]


def _outer(g, engine):
    """The outer model exactly as model_checks.check_hier_gmm builds it (the caller seeds numpy first)."""
    from mimo_amd.distributions import (NormalWishart, TiedGaussiansWithScaledPrecision, Dirichlet, CategoricalWithDirichlet,
                                        TiedGaussiansWithHierarchicalNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfGaussiansWithHierarchicalPrior, BayesianMixtureOfMixtureOfGaussians
    K, M, D = (int(g[k]) for k in ("K", "M", "D"))

    def inner(k):
        gating = CategoricalWithDirichlet(dim=k, prior=Dirichlet(dim=k, alphas=np.ones((k,))))
        hyper = NormalWishart(dim=D, mu=np.zeros((D,)), kappa=1e-2, psi=np.eye(D), nu=D + 1. + 1e-8)
        prior = TiedGaussiansWithScaledPrecision(size=k, dim=D, kappas=1e-2 * np.ones((k,)))
        comps = TiedGaussiansWithHierarchicalNormalWisharts(size=k, dim=D, hyper_prior=hyper, prior=prior, engine=engine)
        return BayesianMixtureOfGaussiansWithHierarchicalPrior(size=k, dim=D, gating=gating, components=comps, engine=engine)
    gating = CategoricalWithDirichlet(dim=M, prior=Dirichlet(dim=M, alphas=np.ones((M,))))
    return BayesianMixtureOfMixtureOfGaussians(cluster_size=M, mixture_size=K, dim=D, gating=gating,
                                               components=[inner(K) for _ in range(M)])


def posteriors(mm):
    return {"galphas": mm.gating.posterior.alphas,
            "post_mus": np.stack([c.components.posterior.mus for c in mm.components]),
            "hyper_psi": np.stack([c.components.hyper_posterior.wishart.psi for c in mm.components]),
            "inner_galphas": np.stack([c.gating.posterior.alphas for c in mm.components])}


@pytest.mark.parametrize("name", FIXTURES)
def test_nested_driver_reproduces_the_reference_fixture_and_the_solo_run(name):
    g = load_golden(name)
    X, seed = g["X"], int(g["seed"])
    npr.seed(seed + 6)
    mm = _outer(g, OracleEngine())
    npr.seed(seed + 7)
    eng = OracleNested()
    assert meanfield_coordinate_descent_nested(mm, X, randomize=True, maxiter=3, maxsubiter=2, maxsubsubiter=2, engine=eng) == []
    assert eng.uploads == 1 and eng.table_uploads == 1       # one copy of the rows; only the random start's (M, N) table goes up
    after = npr.get_state()
    got = posteriors(mm)
    for key, v in got.items():
        assert rel_err(v, g["mom_vi_" + key]) < 1e-7, key
    assert rel_err(expected_responsibilities_nested(mm, X, engine=eng), g["mom_vi_resp"]) < 1e-7

    npr.seed(seed + 6)
    solo = _outer(g, OracleEngine())
    npr.seed(seed + 7)
    solo.meanfield_coordinate_descent(X, randomize=True, maxiter=3, maxsubiter=2, maxsubsubiter=2, progress_bar=False)
    sstate = npr.get_state()
    assert after[0] == sstate[0] and np.array_equal(after[1], sstate[1]) and after[2:] == sstate[2:]   # the same draws
    for key, v in posteriors(solo).items():
        assert rel_err(got[key], v) < 1e-8, key


def test_nested_driver_without_a_random_start_equals_the_solo_run():
    g = load_golden(FIXTURES[0])
    X, seed = g["X"], int(g["seed"])
    models = []
    for nested in (True, False):
        npr.seed(seed + 6)
        mm = _outer(g, OracleEngine())
        npr.seed(seed + 7)
        if nested:
            eng = OracleNested()
            meanfield_coordinate_descent_nested(mm, X, randomize=False, maxiter=2, maxsubiter=3, maxsubsubiter=2, engine=eng)
            assert eng.table_uploads == 0
        else:
            mm.meanfield_coordinate_descent(X, randomize=False, maxiter=2, maxsubiter=3, maxsubsubiter=2, progress_bar=False)
        models.append(posteriors(mm))
    for key in models[0]:
        assert rel_err(models[0][key], models[1][key]) < 1e-8, key


def test_nested_driver_argument_validation():
    g = load_golden(FIXTURES[0])
    npr.seed(1)
    mm = _outer(g, OracleEngine())
    eng = OracleNested()
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_nested(mm.components[0], g["X"], engine=eng)
    with pytest.raises(ValueError):
        expected_responsibilities_nested(object(), g["X"], engine=eng)
    assert eng.uploads == 0
