"""CPU: the device-resident batched VI without a GPU — the header declares the entry points and each fails loudly on a null
context; the argument checks of BatchedHipEngine.vi_set_prior / vi_run / vi_state and of
meanfield_coordinate_descent_batched(resident=True) happen before any library call; the driver's chunk arithmetic, stopping and
write-back against a duck-typed engine that runs the host-native sweep; and the self-check of tests/golden/vi_update_hp.npz:
the host-native route reproduces its 50-digit blocks to 1e-12, so the inputs are known good before a GPU sees them."""
import os
import re

import numpy as np
import numpy.random as npr
import pytest

from conftest import ROOT, load_golden, rel_err
import model_checks as mc
import vi_update_fixture as fx
from oracle_engine import OracleEngine
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched

NAMES = ("mimo_vi_prior_batched", "mimo_vi_run_batched", "mimo_vi_get_batched", "mimo_vi_get_theta_batched")


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES


def test_entry_points_fail_loudly_on_a_null_context():
    lib = _lib.load()
    a = np.ones((1, 1))
    out, n = np.empty(32), np.empty(1, dtype=np.int32)
    p = lambda v: v.ctypes.data
    assert lib.mimo_vi_prior_batched(None, 1, p(a), p(a), p(a), p(a), p(a), p(a)) == _lib.E_INVALID
    assert lib.mimo_vi_run_batched(None, 1, 1, 0.0, 0, p(out), p(n), p(n)) == _lib.E_INVALID
    assert lib.mimo_vi_get_batched(None, 1, p(out)) == _lib.E_INVALID
    assert lib.mimo_vi_get_theta_batched(None, 1, p(out), None) == _lib.E_INVALID


@pytest.mark.parametrize("idx", range(6))
def test_fixture_self_check_host_route_within_1e_12(idx):
    shape = fx.shapes()[idx]
    assert (shape["B"], shape["D"], shape["K"]) == [(3, 1, 1), (3, 2, 4), (2, 3, 17), (2, 16, 5), (2, 12, 33), (1, 7, 128)][idx]
    assert [len(z) for z in shape["rows"]] == [40, 0, 3][:shape["B"]]
    errs = fx.block_errors(fx.host_state(shape), shape)
    for name, e in errs.items():
        assert np.all(e <= 1e-12), (name, float(e.max()))
    # the problem without rows: its posterior is its prior
    if shape["B"] > 1:
        pr, hp = shape["prior"], shape["hp"]
        assert np.array_equal(hp["qc"][1], pr["pc"][1]) and np.array_equal(hp["alpha"][1], pr["alpha0"][1])
        assert np.all(np.abs(hp["vlb"][1]) <= 1e-12 * shape["vlb_scale"][1])


def _offline(rows, D):
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D, eng.shared = None, len(rows), D, False
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_engine_argument_validation():
    eng = _offline([5, 3], 2)
    B, K, D = 2, 3, 2
    good = [np.ones((B, K)), np.zeros((B, K, D)), np.ones((B, K)), np.ones((B, K, D, D)), np.ones((B, K)), np.zeros((B, K))]
    for pos, bad in ((0, np.ones(K)), (0, np.ones((3, K))), (1, np.zeros((B, K, D + 1))), (2, np.ones((B, K + 1))),
                     (3, np.ones((B, K, D))), (4, np.ones((B, 1))), (5, np.zeros((K, B))),
                     (0, np.full((B, K), np.nan)), (3, np.full((B, K, D, D), np.inf)), (5, np.full((B, K), -np.inf))):
        args = list(good)
        args[pos] = bad
        with pytest.raises(ValueError):
            eng.vi_set_prior(*args)
    for K_, iters, tol in ((0, 1, 0.), (3, 0, 0.), (3, 1, -1.), (3, 1, float('nan'))):
        with pytest.raises(ValueError):
            eng.vi_run(K_, iters, tol)
    with pytest.raises(ValueError):
        eng.vi_state(0)
    # well-formed arguments pass the validation (and then need the library: the offline object has none)
    for call in (lambda: eng.vi_set_prior(*good), lambda: eng.vi_run(K, 2, 1e-8), lambda: eng.vi_state(K)):
        with pytest.raises(AttributeError):
            call()


def test_driver_refuses_what_the_resident_loop_does_not_cover():
    from mimo_amd.distributions import TiedNormalWisharts, TiedGaussiansWithNormalWisharts
    from mimo_amd.mixtures import BayesianMixtureOfGaussians
    engine = OracleEngine()
    g = load_golden("gibbs_c1_trace")
    models = [mc.build_gmm(g, engine)[1] for _ in range(2)]
    data = [g["X"], g["X"][:100]]
    gi = load_golden("ilr_svi_dx2_dy1_k8")
    ilrs = [mc.build_ilr(gi, engine)[1] for _ in range(2)]
    gs = load_golden("gmm_c3_d8_k32_stick")
    sticks = [mc.build_gmm(gs, engine)[1] for _ in range(2)]
    K, D = int(g["K"]), int(g["D"])
    prior = TiedNormalWisharts(size=K, dim=D, **{k: g["prior_" + k] for k in ("mus", "kappas", "psis", "nus")})
    tied = [BayesianMixtureOfGaussians(gating=mc.make_gating(g, K)[1],
                                       components=TiedGaussiansWithNormalWisharts(size=K, dim=D, prior=prior, engine=engine),
                                       engine=engine) for _ in range(2)]

    class NoUpload:
        device = 0

        def upload(self, arrays):
            raise AssertionError("the batch was uploaded before the models were checked")
    state = npr.get_state()
    for ms, ds, kw, word in ((models, data, dict(sample_likelihood=True), "sample_likelihood"),
                             (models, data, dict(), "sample_likelihood"),                 # (the default draws)
                             (ilrs, [(gi["X"], gi["Y"])] * 2, dict(sample_likelihood=False), "BayesianMixtureOfGaussians"),
                             (sticks, [gs["X"]] * 2, dict(sample_likelihood=False), "gating"),
                             (tied, data, dict(sample_likelihood=False), "tied")):
        with pytest.raises(ValueError, match=word):
            meanfield_coordinate_descent_batched(ms, ds, resident=True, engine=NoUpload(), **kw)
    after = npr.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # nothing was drawn


class FakeResident:
    """Duck-typed batch on the CPU oracle: what meanfield_coordinate_descent_batched uses of BatchedHipEngine on both routes.
    vi_run runs the host-native sweep per problem, with the loop's rules (a stopped problem is left alone and appends nothing)."""
    device = 0

    def __init__(self):
        self.runs, self.state_reads, self.prior_sets = [], 0, 0

    def upload(self, arrays):
        self.engs = []
        for z in arrays:
            e = OracleEngine()
            e.upload(np.asarray(z, dtype=float))
            self.engs.append(e)
        self.B, self.D = len(arrays), arrays[0].shape[1]
        self.row_off = np.concatenate([[0], np.cumsum([len(z) for z in arrays])]).astype(np.int64)
        self.prior = self.S = None

    def estep(self, c, b, W, stats=True, **kw):
        out = [e.estep(c[i], b[i], W[i]) for i, e in enumerate(self.engs)]
        self.S = [S for S, _ in out]
        return list(self.S), np.stack([sc for _, sc in out])

    def weighted_stats(self, tables=None, K=None):
        self.S = [e.weighted_stats(t) for e, t in zip(self.engs, tables)]
        return list(self.S)

    def vi_set_prior(self, *prior):
        assert self.S is not None
        self.prior = [np.array(v, dtype=float) for v in prior]
        self.active, self.blocks, self.last = [True] * self.B, [None] * self.B, [None] * self.B
        self.prior_sets += 1

    def vi_run(self, K, iters, tol):
        assert self.prior is not None
        self.runs.append(int(iters))
        trace = np.full((iters, self.B), np.nan)
        n_done = np.zeros(self.B, dtype=np.int32)
        for it in range(iters):
            for i in range(self.B):
                if not self.active[i]:
                    continue
                S = self.S[i]
                blk = fx.host_sweep(K, self.D, tuple(v[i] for v in self.prior), S.n, S.sx, S.sxx)
                self.S[i], sc = self.engs[i].estep(blk["c_total"], blk["bb"], blk["W"])
                v = float(blk["vlb"][0] + blk["vlb"][1]) + sc[0]
                trace[it, i] = v
                n_done[i] += 1
                if self.last[i] is not None and abs(v - self.last[i]) < tol:
                    self.active[i] = False
                self.blocks[i], self.last[i] = blk, v
        return trace, n_done, np.zeros(self.B, dtype=np.int32)

    def vi_state(self, K):
        self.state_reads += 1
        return {name: np.stack([blk[name] for blk in self.blocks]) for name in self.blocks[0]}


def _gmms(B):
    g = load_golden("gmm_c1_d2_k4_dir")
    engine = OracleEngine()
    models = []
    for _ in range(B):
        kind, m = mc.build_gmm(g, engine)
        mc.load_gmm_state(m, g, kind)
        models.append(m)
    rng = np.random.default_rng(5)
    data = [g["X"], g["X"][:37] + 0.5, g["X"] + 0.1 * rng.standard_normal(g["X"].shape)][:B]
    return models, data


@pytest.mark.parametrize("maxiter,chunk,runs", [(7, 3, [3, 3, 1]), (6, 8, [6]), (4, 1, [1, 1, 1, 1]), (0, 8, [])])
def test_driver_chunks_and_writes_back_like_the_host_route(maxiter, chunk, runs):
    models, data = _gmms(3)
    fake = FakeResident()
    npr.seed(3)
    vlbs = meanfield_coordinate_descent_batched(models, data, randomize=False, maxiter=maxiter, tol=0., sample_likelihood=False,
                                                engine=fake, resident=True, chunk=chunk)
    assert fake.runs == runs and [len(v) for v in vlbs] == [maxiter] * 3
    assert fake.prior_sets == (1 if maxiter else 0) and fake.state_reads == (1 if maxiter else 0)
    ref, _ = _gmms(3)
    host = meanfield_coordinate_descent_batched(ref, data, randomize=False, maxiter=maxiter, tol=0., sample_likelihood=False,
                                                engine=FakeResident())
    assert vlbs == host                                           # the same native sweep on both routes
    for m, r in zip(models, ref):
        assert np.array_equal(m.gating.posterior.alphas, r.gating.posterior.alphas)
        for a, b in zip(m.components.posterior.params, r.components.posterior.params):
            assert np.array_equal(a, b)
        for a, b in zip(m.components.posterior.nat_param, r.components.posterior.nat_param):
            assert np.array_equal(a, b)
        for a, b in zip(m.canonical_expected(), r.canonical_expected()):
            assert np.array_equal(a, b)
        assert m._vlb_prior_terms() == r._vlb_prior_terms()


def test_driver_stops_in_chunks_where_the_host_route_stops():
    models, data = _gmms(3)
    ref, _ = _gmms(3)
    kw = dict(randomize=True, maxiter=120, tol=1e-2, sample_likelihood=False)
    npr.seed(11)
    host = meanfield_coordinate_descent_batched(ref, data, engine=FakeResident(), **kw)
    assert len(set(len(v) for v in host)) > 1 and max(len(v) for v in host) < 120
    fake = FakeResident()
    npr.seed(11)
    vlbs = meanfield_coordinate_descent_batched(models, data, engine=fake, resident=True, chunk=4, **kw)
    assert vlbs == host
    longest = max(len(v) for v in host)
    assert fake.runs == [4] * (-(-longest // 4))                  # no call behind the last problem's stop
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched(models, data, engine=FakeResident(), resident=True, chunk=0, **kw)
