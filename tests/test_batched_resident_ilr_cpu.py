"""CPU: the device-resident batched VI for mixtures of linear-Gaussian experts without a GPU — the header declares the entry
points and each fails loudly on a null context; the self-check of tests/golden/vi_ilr_update_hp.npz (the host yardstick
reproduces its 50-digit blocks to 1e-12, so the inputs are known good before a GPU sees them); the argument checks of
BatchedHipEngine.vi_ilr_set_prior / vi_ilr_run / vi_ilr_state and of meanfield_coordinate_descent_batched_ilr happen before any
library call; the driver's chunk arithmetic and write-back against a duck-typed engine that runs the host route per problem."""
import os
import re

import numpy as np
import numpy.random as npr
import pytest

from conftest import ROOT, load_golden
import model_checks as mc
import vi_ilr_update_fixture as fx
from oracle_engine import OracleEngine
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched, meanfield_coordinate_descent_batched_ilr

NAMES = ("mimo_vi_ilr_prior_batched", "mimo_vi_ilr_run_batched", "mimo_vi_ilr_get_batched")
SHAPES = [(3, 1, 1, 1, 'dirichlet'), (3, 1, 1, 6, 'dirichlet'), (2, 2, 1, 17, 'stick-breaking'), (2, 8, 4, 5, 'stick-breaking'),
          (2, 15, 1, 2, 'dirichlet'), (2, 1, 15, 3, 'stick-breaking'), (2, 1, 3, 33, 'dirichlet'), (1, 1, 1, 128, 'stick-breaking')]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES


def test_entry_points_fail_loudly_on_a_null_context():
    lib = _lib.load()
    a = np.ones((1, 4))
    out, n = np.empty(64), np.empty(1, dtype=np.int32)
    p = lambda v: v.ctypes.data
    assert lib.mimo_vi_ilr_prior_batched(None, 1, 1, 1, 0, *([p(a)] * 12)) == _lib.E_INVALID
    assert lib.mimo_vi_ilr_run_batched(None, 1, 1, 0.0, 0, p(out), p(n), p(n)) == _lib.E_INVALID
    assert lib.mimo_vi_ilr_get_batched(None, 1, p(out)) == _lib.E_INVALID


@pytest.mark.parametrize("idx", range(8))
def test_fixture_self_check_host_route_within_1e_12(idx):
    shape = fx.shapes()[idx]
    assert (shape["B"], shape["dx"], shape["dy"], shape["K"], shape["gating"]) == SHAPES[idx]
    assert [len(z) for z in shape["rows"]] == [40, 0, 3][:shape["B"]]
    host = fx.host_state(shape)
    errs = fx.block_errors(host, shape)
    for name, e in errs.items():
        assert np.all(e <= 1e-12), (name, float(e.max()))
    # the problem without rows: its posterior is its prior, its terms are 0 within 1e-12 of their scale
    if shape["B"] > 1:
        pr, hp = shape["prior"], shape["hp"]
        assert np.array_equal(hp["qc"][1], pr["basis"][2][1]) and np.array_equal(hp["m_Kq"][1], pr["experts"][1][1])
        assert np.array_equal(hp["m_a"][1], pr["experts"][0][1]) and np.array_equal(hp["g0"][1], pr["g0"][1])
        assert np.all(np.abs(hp["vlb"][1]) <= 1e-12 * shape["vlb_scale"][1])
        assert np.all(np.abs(host["vlb"][1]) <= 1e-12 * shape["vlb_scale"][1])


def _offline(rows, D):
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D, eng.shared = None, len(rows), D, False
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_engine_argument_validation():
    B, K, dx, dy = 2, 3, 2, 1
    dc = dx + 1
    eng = _offline([5, 3], dx + dy)
    basis = lambda: [np.zeros((B, K, dx)), np.ones((B, K)), np.ones((B, K, dx, dx)), np.ones((B, K)), np.zeros((B, K))]
    experts = lambda: [np.zeros((B, K, dy, dc)), np.ones((B, K, dc, dc)), np.ones((B, K, dy, dy)), np.ones((B, K)), np.zeros((B, K))]
    g = np.ones((B, K))
    bad_calls = [("gamma", g, None, basis(), experts()), ("dirichlet", g, g, basis(), experts()),
                 ("stick-breaking", g, None, basis(), experts()), ("dirichlet", np.ones(K), None, basis(), experts()),
                 ("dirichlet", np.ones((3, K)), None, basis(), experts()), ("stick-breaking", g, np.ones((B, K + 1)), basis(), experts()),
                 ("dirichlet", g, None, basis()[:4], experts()), ("dirichlet", np.full((B, K), np.nan), None, basis(), experts())]
    for pos, bad in ((0, np.zeros((B, K, dx + 1))), (0, np.zeros((B, K))), (1, np.ones((B, K + 1))), (2, np.ones((B, K, dx))),
                     (4, np.zeros((K, B))), (2, np.full((B, K, dx, dx), np.inf))):
        bs = basis()
        bs[pos] = bad
        bad_calls.append(("dirichlet", g, None, bs, experts()))
    for pos, bad in ((0, np.zeros((B, K, dy, dx))), (0, np.zeros((B, K, dc))), (1, np.ones((B, K, dx, dx))), (2, np.ones((B, K, dy))),
                     (3, np.ones((B, 1))), (4, np.full((B, K), -np.inf)), (0, np.zeros((B, K, dy + 1, dc)))):      # (dx + dy != Dz)
        ex = experts()
        ex[pos] = bad
        bad_calls.append(("stick-breaking", g, g, basis(), ex))
    for args in bad_calls:
        with pytest.raises(ValueError):
            eng.vi_ilr_set_prior(*args)
    for K_, iters, tol in ((0, 1, 0.), (3, 0, 0.), (3, 1, -1.), (3, 1, float('nan'))):
        with pytest.raises(ValueError):
            eng.vi_ilr_run(K_, iters, tol)
    with pytest.raises(ValueError):
        eng.vi_ilr_state(0)
    with pytest.raises(ValueError):
        eng.vi_ilr_state(K)                      # no ILR prior block was set
    # well-formed arguments pass the validation (and then need the library: the offline object has none)
    for call in (lambda: eng.vi_ilr_set_prior("dirichlet", g, None, basis(), experts()),
                 lambda: eng.vi_ilr_set_prior("stick-breaking", g, g, basis(), experts()), lambda: eng.vi_ilr_run(K, 2, 1e-8)):
        with pytest.raises(AttributeError):
            call()


def _ilrs(name, B, load=True):
    g = load_golden(name)
    engine = OracleEngine()
    models = []
    for _ in range(B):
        kind, m = mc.build_ilr(g, engine)
        if load:
            mc.load_ilr_state(m, g, kind)
        models.append(m)
    rng = np.random.default_rng(5)
    X, Y = g["X"], g["Y"]
    data = [(X, Y), (X[:37] + 0.5, Y[:37]), (X, Y + 0.1 * rng.standard_normal(Y.shape))][:B]
    return models, data


def test_driver_refuses_what_the_resident_loop_does_not_cover():
    from mimo_amd.distributions import (StackedMatrixNormalWisharts, StackedLinearGaussiansWithMatrixNormalWisharts,
                                        TiedMatrixNormalWisharts, TiedLinearGaussiansWithMatrixNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfLinearGaussians
    engine = OracleEngine()
    gi = load_golden("ilr_dx1_dy1_k6_dir")
    K, dx, dy = int(gi["K"]), gi["X"].shape[1], gi["Y"].shape[1]
    data = [(gi["X"], gi["Y"])] * 2
    good = mc.build_ilr(gi, engine)[1]

    def variant(experts):
        basis = mc.build_ilr(gi, engine)[1].basis
        return BayesianMixtureOfLinearGaussians(size=K, input_dim=dx, output_dim=dy, gating=mc.make_gating(gi, K)[1], basis=basis,
                                                models=experts, engine=engine)
    mp = {k: gi["mprior_" + k] for k in ("Ms", "Ks", "psis", "nus")}
    plain = StackedMatrixNormalWisharts(K, dx, dy, Ms=mp["Ms"][:, :, :dx], Ks=mp["Ks"][:, :dx, :dx], psis=mp["psis"], nus=mp["nus"])
    nonaffine = variant(StackedLinearGaussiansWithMatrixNormalWisharts(K, dx, dy, plain, affine=False, engine=engine))
    tied = variant(TiedLinearGaussiansWithMatrixNormalWisharts(K, dx + 1, dy, TiedMatrixNormalWisharts(K, dx + 1, dy, **mp),
                                                              affine=True, engine=engine))
    gs = load_golden("ilr_dx1_dy1_k50_stick")
    stick = mc.build_ilr(gs, engine)[1]
    gg = load_golden("gibbs_c1_trace")
    gmms = [mc.build_gmm(gg, engine)[1] for _ in range(2)]

    class NoUpload:
        device = 0

        def upload(self, arrays):
            raise AssertionError("the batch was uploaded before the models were checked")
    state = npr.get_state()
    for ms, ds, word in (([good, nonaffine], data, "model 1.*affine"), ([tied, good], data, "model 0.*[Tt]ied"),
                         (gmms, [gg["X"]] * 2, "model 0.*BayesianMixtureOfLinearGaussians")):
        with pytest.raises(ValueError, match=word):
            meanfield_coordinate_descent_batched_ilr(ms, ds, engine=NoUpload())
    # a mixed-gating batch (sizes aside: the gating kinds are compared first)
    with pytest.raises(ValueError, match="one gating kind"):
        meanfield_coordinate_descent_batched_ilr([good, stick], [data[0], (gs["X"], gs["Y"])], engine=NoUpload())
    after = npr.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # nothing was drawn
    # the GMM driver keeps refusing ILR models under resident=True
    with pytest.raises(ValueError, match="BayesianMixtureOfGaussians"):
        meanfield_coordinate_descent_batched([good, mc.build_ilr(gi, engine)[1]], data, resident=True, sample_likelihood=False,
                                             engine=NoUpload())


class FakeResidentIlr:
    """Duck-typed batch on the CPU oracle: what both drivers use of BatchedHipEngine.  vi_ilr_run runs the host route per problem
    (a model built on the uploaded priors: _update_from_stats, canonical_expected, the three terms), with the loop's rules (a
    stopped problem is left alone and appends nothing)."""
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
        self.models = self.S = None

    def estep(self, c, b, W, stats=True, **kw):
        out = [e.estep(c[i], b[i], W[i]) for i, e in enumerate(self.engs)]
        self.S = [S for S, _ in out]
        return list(self.S), np.stack([sc for _, sc in out])

    def weighted_stats(self, tables=None, K=None):
        self.S = [e.weighted_stats(t) for e, t in zip(self.engs, tables)]
        return list(self.S)

    def vi_ilr_set_prior(self, gating, g0, g1, basis, experts):
        assert self.S is not None
        K, dx, dy = g0.shape[1], basis[0].shape[2], experts[0].shape[2]
        assert dx + dy == self.D
        state = npr.get_state()                  # (the models' constructors draw their likelihoods)
        self.models = [fx.build_model(K, dx, dy, gating, g0[i], None if g1 is None else g1[i], tuple(v[i] for v in basis),
                                      tuple(v[i] for v in experts)) for i in range(self.B)]
        npr.set_state(state)
        self.active, self.blocks, self.last = [True] * self.B, [None] * self.B, [None] * self.B
        self.prior_sets += 1

    def vi_ilr_run(self, K, iters, tol):
        assert self.models is not None
        self.runs.append(int(iters))
        trace = np.full((iters, self.B), np.nan)
        n_done = np.zeros(self.B, dtype=np.int32)
        for it in range(iters):
            for i in range(self.B):
                if not self.active[i]:
                    continue
                S = self.S[i]
                blk = fx.host_update(self.models[i], S.n, S.sx, S.sxx)
                self.S[i], sc = self.engs[i].estep(blk["c_total"], blk["j_bb"], blk["j_W"])
                v = float(blk["vlb"][0] + blk["vlb"][1] + blk["vlb"][2]) + sc[0]
                trace[it, i] = v
                n_done[i] += 1
                if self.last[i] is not None and abs(v - self.last[i]) < tol:
                    self.active[i] = False
                self.blocks[i], self.last[i] = blk, v
        return trace, n_done, np.zeros(self.B, dtype=np.int32)

    def vi_ilr_state(self, K):
        self.state_reads += 1
        return {name: np.stack([blk[name] for blk in self.blocks]) for name in self.blocks[0]}


@pytest.mark.parametrize("name", ["ilr_dx1_dy1_k6_dir", "ilr_dx1_dy1_k50_stick"])
@pytest.mark.parametrize("maxiter,chunk,runs", [(7, 3, [3, 3, 1]), (6, 8, [6]), (4, 1, [1, 1, 1, 1]), (0, 8, [])])
def test_driver_chunks_and_writes_back_like_the_host_route(name, maxiter, chunk, runs):
    models, data = _ilrs(name, 3)
    fake = FakeResidentIlr()
    npr.seed(3)
    vlbs = meanfield_coordinate_descent_batched_ilr(models, data, randomize=False, maxiter=maxiter, tol=0., engine=fake, chunk=chunk)
    assert fake.runs == runs and [len(v) for v in vlbs] == [maxiter] * 3
    assert fake.prior_sets == (1 if maxiter else 0) and fake.state_reads == (1 if maxiter else 0)
    ref, _ = _ilrs(name, 3)
    host = meanfield_coordinate_descent_batched(ref, data, randomize=False, maxiter=maxiter, tol=0., sample_likelihood=False,
                                                engine=FakeResidentIlr())
    assert vlbs == host                                           # the same host route on both sides
    for m, r in zip(models, ref):
        for a, b in zip(np.atleast_2d(mc.gating_posterior(m.gating, mc.gating_of(load_golden(name), "gprior")[0])),
                        np.atleast_2d(mc.gating_posterior(r.gating, mc.gating_of(load_golden(name), "gprior")[0]))):
            assert np.array_equal(a, b)
        for blk in ("basis", "models"):
            pm, pr = getattr(m, blk).posterior, getattr(r, blk).posterior
            for a, b in zip(pm.params, pr.params):
                assert np.array_equal(a, b)
            for a, b in zip(pm.nat_param, pr.nat_param):
                assert np.array_equal(a, b)
            for a, b in zip(pm.expected_statistics(), pr.expected_statistics()):      # (the memos)
                assert np.array_equal(a, b)
            assert np.array_equal(pm._half_logdet_psi(), pr._half_logdet_psi())
        if maxiter:
            assert "canon_affine" in m.models.posterior._memo and m.basis.posterior._memo.get("native")
        for a, b in zip(m.canonical_expected(), r.canonical_expected()):
            assert np.array_equal(a, b)
        assert m._vlb_prior_terms() == r._vlb_prior_terms()


def test_driver_stops_in_chunks_where_the_host_route_stops():
    models, data = _ilrs("ilr_dx1_dy1_k6_dir", 3, load=False)
    ref, _ = _ilrs("ilr_dx1_dy1_k6_dir", 3, load=False)
    kw = dict(randomize=True, maxiter=150, tol=1e-2)
    npr.seed(11)
    host = meanfield_coordinate_descent_batched(ref, data, engine=FakeResidentIlr(), sample_likelihood=False, **kw)
    assert len(set(len(v) for v in host)) > 1 and max(len(v) for v in host) < 150
    fake = FakeResidentIlr()
    npr.seed(11)
    vlbs = meanfield_coordinate_descent_batched_ilr(models, data, engine=fake, chunk=4, **kw)
    assert vlbs == host
    longest = max(len(v) for v in host)
    assert fake.runs == [4] * (-(-longest // 4))                  # no call behind the last problem's stop
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched_ilr(models, data, engine=FakeResidentIlr(), chunk=0, **kw)
