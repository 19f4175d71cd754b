"""CPU: the device-resident batched SVI without a GPU — the header declares the entry points and each fails loudly on a null
context; the argument checks of BatchedHipEngine.svi_set_state / svi_run (and their _ilr_ forms) and of
meanfield_stochastic_descent_batched(resident=True) happen before any library call, upload or draw; the driver's chunk
arithmetic, the order in which it consumes Python's and NumPy's streams, and its write-back against a duck-typed engine whose
svi_run is the host route (_svi_step per problem)."""
import copy
import os
import random
import re

import numpy as np
import numpy.random as npr
import pytest

from conftest import ROOT, load_golden
import model_checks as mc
import vi_ilr_update_fixture as fxi
from oracle_engine import OracleEngine
from test_batched_resident_ilr_cpu import _ilrs
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched, meanfield_stochastic_descent_batched

NAMES = ("mimo_svi_state_batched", "mimo_svi_ilr_state_batched", "mimo_svi_run_batched", "mimo_svi_ilr_run_batched")


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mimo_hip.h")).read()
    assert re.search(r"#define\s+MIMO_F_SVI_RESIDENT_START\s+0x400\b", text) and _lib.F_SVI_RESIDENT_START == 0x400
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES


def test_entry_points_fail_loudly_on_a_null_context():
    lib = _lib.load()
    a, idx = np.ones((1, 4)), np.zeros(4, dtype=np.int64)
    out, n = np.empty(64), np.empty(1, dtype=np.int32)
    p = lambda v: v.ctypes.data
    assert lib.mimo_svi_state_batched(None, 1, *([p(a)] * 5), p(n)) == _lib.E_INVALID
    assert lib.mimo_svi_ilr_state_batched(None, 1, *([p(a)] * 10), p(n)) == _lib.E_INVALID
    for run in (lib.mimo_svi_run_batched, lib.mimo_svi_ilr_run_batched):
        assert run(None, 1, 1, 0.5, p(a), p(idx), p(idx), None, 0, p(out), p(n), p(n)) == _lib.E_INVALID


def _offline(rows, D):
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D, eng.shared = None, len(rows), D, False
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_engine_argument_validation():
    B, K, D = 2, 3, 2
    eng = _offline([5, 3], D)
    good = [np.ones((B, K)), np.zeros((B, K, D)), np.ones((B, K)), np.ones((B, K, D, D)), np.ones((B, K))]
    for pos, bad in ((0, np.ones(K)), (0, np.ones((3, K))), (1, np.zeros((B, K, D + 1))), (2, np.ones((B, K + 1))),
                     (3, np.ones((B, K, D))), (4, np.ones((B, 1))), (0, np.full((B, K), np.nan)), (3, np.full((B, K, D, D), np.inf))):
        args = list(good)
        args[pos] = bad
        with pytest.raises(ValueError):
            eng.svi_set_state(*args)
    # the ILR state: needs the dimensions of vi_ilr_set_prior
    dx, dy, dc = 1, 1, 2
    basis = lambda: [np.zeros((B, K, dx)), np.ones((B, K)), np.ones((B, K, dx, dx)), np.ones((B, K))]
    experts = lambda: [np.zeros((B, K, dy, dc)), np.ones((B, K, dc, dc)), np.ones((B, K, dy, dy)), np.ones((B, K))]
    g = np.ones((B, K))
    with pytest.raises(ValueError, match="vi_ilr_set_prior"):
        eng.svi_ilr_set_state(g, None, basis(), experts())
    eng._vi_ilr_dims = (dx, dy)
    bad_calls = [(np.ones(K), None, basis(), experts()), (np.ones((3, K)), None, basis(), experts()), (g, np.ones((B, K + 1)), basis(), experts()),
                 (g, None, basis()[:3], experts()), (g, None, basis(), experts() + [g]), (np.full((B, K), np.nan), None, basis(), experts())]
    for pos, bad in ((0, np.zeros((B, K, dx + 1))), (2, np.ones((B, K, dx))), (3, np.full((B, K), np.inf))):
        bs = basis()
        bs[pos] = bad
        bad_calls.append((g, None, bs, experts()))
    for pos, bad in ((0, np.zeros((B, K, dy, dx))), (1, np.ones((B, K, dx, dx))), (2, np.ones((B, K, dy))), (3, np.ones((B, 1)))):
        ex = experts()
        ex[pos] = bad
        bad_calls.append((g, g, basis(), ex))
    for args in bad_calls:
        with pytest.raises(ValueError):
            eng.svi_ilr_set_state(*args)

    scale, sizes = np.array([0.4, 1.0]), np.array([2, 3])
    sel = lambda: [np.array([0, 4]), np.array([2, 1, 0])]
    for run in (eng.svi_run, eng.svi_ilr_run):
        bad_runs = [dict(K=0), dict(iters=0), dict(step_size=0.), dict(step_size=1.5), dict(step_size=float('nan')),
                    dict(scale=np.array([0.4])), dict(scale=np.array([0.4, 0.])), dict(scale=np.array([-1., 1.])),
                    dict(scale=np.array([0.4, np.inf])), dict(scale=np.array([np.nan, 1.])),
                    dict(batch_sizes=np.array([2])), dict(batch_sizes=np.array([2, -1])), dict(batch_sizes=np.array([2., 3.])),
                    dict(rows=[sel()]),                                        # one selection for two iterations
                    dict(rows=[sel(), sel()], resident_start=True),            # the resident start takes iters - 1
                    dict(rows=[sel(), sel()[:1]]),                             # a problem's rows are missing
                    dict(rows=[sel(), [np.array([0, 4]), np.array([2, 1])]]),  # rows against sel_off
                    dict(rows=[sel(), [np.array([0, 5]), np.array([2, 1, 0])]]),   # an index outside [0, N_b)
                    dict(rows=[sel(), [np.array([0, -1]), np.array([2, 1, 0])]]),
                    dict(rows=[sel(), [np.array([0., 4.]), np.array([2, 1, 0])]]),
                    dict(rows=[sel(), sel()], seeds=[1, 2]),                   # indices and seeds
                    dict(rows=None, seeds=[1]), dict(rows=None, seeds=None)]
        for bad in bad_runs:
            kw = dict(K=K, iters=2, step_size=0.5, scale=scale, batch_sizes=sizes, rows=[sel(), sel()])
            kw.update(bad)
            with pytest.raises(ValueError):
                run(**kw)
        # well-formed arguments pass the validation (and then need the library: the offline object has none)
        for kw in (dict(rows=[sel(), sel()]), dict(rows=[sel()], resident_start=True), dict(rows=None, seeds=[1, 2]),
                   dict(rows=[np.concatenate(sel()), sel()]), dict(rows=None, seeds=[1, 2], scale=np.array([0.4, 7.5]))):
            with pytest.raises(AttributeError):
                run(**dict(dict(K=K, iters=2, step_size=0.5, scale=scale, batch_sizes=sizes), **kw))
    for call in (lambda: eng.svi_set_state(*good), lambda: eng.svi_ilr_set_state(g, None, basis(), experts()),
                 lambda: eng.svi_ilr_set_state(g, g, basis(), experts())):
        with pytest.raises(AttributeError):
            call()


class NoUpload:
    device = 0

    def upload(self, arrays):
        raise AssertionError("the batch was uploaded before the models were checked")


def test_driver_refuses_what_the_resident_loop_does_not_cover():
    from mimo_amd.distributions import (StackedMatrixNormalWisharts, StackedLinearGaussiansWithMatrixNormalWisharts,
                                        TiedNormalWisharts, TiedGaussiansWithNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfGaussians, BayesianMixtureOfLinearGaussians
    engine = OracleEngine()
    g = load_golden("gibbs_c1_trace")
    gmms = [mc.build_gmm(g, engine)[1] for _ in range(2)]
    gdata = [g["X"], g["X"][:100]]
    K, D = int(g["K"]), int(g["D"])
    prior = TiedNormalWisharts(size=K, dim=D, **{k: g["prior_" + k] for k in ("mus", "kappas", "psis", "nus")})
    tied = [BayesianMixtureOfGaussians(gating=mc.make_gating(g, K)[1],
                                       components=TiedGaussiansWithNormalWisharts(size=K, dim=D, prior=prior, engine=engine),
                                       engine=engine) for _ in range(2)]
    gi = load_golden("ilr_dx1_dy1_k6_dir")
    Ki, dx, dy = int(gi["K"]), gi["X"].shape[1], gi["Y"].shape[1]
    idata = [(gi["X"], gi["Y"])] * 2
    good = mc.build_ilr(gi, engine)[1]
    mp = {k: gi["mprior_" + k] for k in ("Ms", "Ks", "psis", "nus")}
    plain = StackedMatrixNormalWisharts(Ki, dx, dy, Ms=mp["Ms"][:, :, :dx], Ks=mp["Ks"][:, :dx, :dx], psis=mp["psis"], nus=mp["nus"])
    nonaffine = [BayesianMixtureOfLinearGaussians(
        size=Ki, input_dim=dx, output_dim=dy, gating=mc.make_gating(gi, Ki)[1], basis=mc.build_ilr(gi, engine)[1].basis,
        models=StackedLinearGaussiansWithMatrixNormalWisharts(Ki, dx, dy, copy.deepcopy(plain), affine=False, engine=engine),
        engine=engine) for _ in range(2)]
    gs = load_golden("ilr_dx1_dy1_k50_stick")
    stick = mc.build_ilr(gs, engine)[1]
    off = dict(sample_likelihood=False)
    npstate, pystate = npr.get_state(), random.getstate()
    for ms, ds, kw, word in ((gmms, gdata, dict(sample_likelihood=True), "model 0.*sample_likelihood"),
                             (gmms, gdata, dict(), "sample_likelihood"),                     # (the default draws)
                             ([good, good], idata, dict(sample_likelihood=True), "sample_likelihood"),
                             (tied, gdata, off, "model 0.*tied"),
                             (nonaffine, idata, off, "model 0.*affine"),
                             ([good, stick], [idata[0], (gs["X"], gs["Y"])], off, "one gating kind"),
                             (gmms, gdata, dict(off, batch_size=101), "model 1.*batch_size = 101"),   # index_rng='host', N_1 = 100
                             (gmms, gdata, dict(off, index_rng='device'), "device"),
                             (gmms, gdata, dict(off, chunk=0), "chunk"),
                             (gmms, gdata, dict(off, index_rng='philox', seeds=[1]), "seeds")):
        with pytest.raises(ValueError, match=word):
            meanfield_stochastic_descent_batched(ms, ds, resident=True, maxiter=3, engine=NoUpload(), **kw)
    after = npr.get_state()
    assert np.array_equal(npstate[1], after[1]) and npstate[2:] == after[2:] and random.getstate() == pystate      # nothing was drawn
    # index_rng='philox' draws with replacement: a minibatch larger than the data set passes the checks (and reaches the upload)
    with pytest.raises(AssertionError, match="uploaded"):
        meanfield_stochastic_descent_batched(gmms, gdata, resident=True, maxiter=3, engine=NoUpload(), batch_size=101,
                                             index_rng='philox', seeds=[1, 2], **off)


def _gmm_blocks(model):
    """The blocks of a mixture of Gaussians' posteriors under the names of BatchedHipEngine.vi_state that the write-back reads."""
    post = model.components.posterior
    o = dict(alpha=np.array(model.gating.posterior.alphas, dtype=float))
    o["qa"], o["qb"], o["qc"], o["qd"] = (np.asarray(v, dtype=float) for v in post.nat_param)
    o["mus"], _, o["psis"], o["nus"] = (np.asarray(v, dtype=float) for v in post.params)
    o["hld"] = np.asarray(post._half_logdet_psi(), dtype=float)
    o["cc"], o["bb"], o["W"] = (np.asarray(v, dtype=float) for v in post.canonical_expected())
    E = post.expected_statistics()
    o["E2"], o["E4"] = np.asarray(E[1], dtype=float), np.asarray(E[3], dtype=float)
    return o


class FakeResidentSvi:
    """Duck-typed batch on the CPU oracle: what meanfield_stochastic_descent_batched uses of BatchedHipEngine on both routes.
    The resident calls run the host route on `shadow`, models built as the driver's were: svi_set_state checks
    that the uploaded posterior is theirs, svi_run is _svi_step per problem and iteration, the state is read off their blocks."""
    device = 0

    def __init__(self, shadow=None):
        self.shadow = shadow
        self.runs, self.state_reads, self.prior_sets, self.state_sets = [], 0, 0, 0
        self.batches, self.tables = [], []

    def upload(self, arrays):
        self.Z = [np.asarray(z, dtype=float) for z in arrays]
        self.engs = []
        for z in self.Z:
            e = OracleEngine()
            e.upload(z)
            self.engs.append(e)
        self.B, self.D = len(arrays), arrays[0].shape[1]
        self.row_off = np.concatenate([[0], np.cumsum([len(z) for z in arrays])]).astype(np.int64)
        self.S = None

    def _subset(self, i, rows, canon):
        e = OracleEngine()
        e.upload(self.Z[i][np.asarray(rows)])
        return e.estep(*canon)[0]

    def estep(self, c, b, W, stats=True, rows=None, **kw):
        if rows is not None:
            self.batches.append([np.array(r) for r in rows])
            self.S = [self._subset(i, rows[i], (c[i], b[i], W[i])) for i in range(self.B)]
            return list(self.S), None
        out = [e.estep(c[i], b[i], W[i]) for i, e in enumerate(self.engs)]
        return ([S for S, _ in out] if stats else None), np.stack([sc for _, sc in out])

    def weighted_stats(self, tables=None, K=None):
        self.tables.append([np.array(t) for t in tables])
        self.S = [e.weighted_stats(t) for e, t in zip(self.engs, tables)]
        return list(self.S)

    # ---- the resident calls
    def vi_set_prior(self, alpha0, *blocks):
        assert all(np.array_equal(alpha0[i], m.gating.prior.alphas) for i, m in enumerate(self.shadow))
        self.prior_sets += 1

    def vi_ilr_set_prior(self, gating, g0, g1, basis, experts):
        assert (g1 is not None) == (gating == 'stick-breaking') and len(basis) == 5 and len(experts) == 5
        self.prior_sets += 1

    def svi_set_state(self, alpha, qa, qb, qc, qd):
        for i, m in enumerate(self.shadow):
            assert np.array_equal(alpha[i], m.gating.posterior.alphas)
            for got, want in zip((qa, qb, qc, qd), m.components.posterior.nat_param):
                assert np.array_equal(got[i], want)
        self.state_sets += 1
        return np.zeros(self.B, dtype=np.int32)

    def svi_ilr_set_state(self, g0, g1, basis, experts):
        for i, m in enumerate(self.shadow):
            blk = fxi.model_blocks(m)
            assert np.array_equal(g0[i], blk["g0"]) and (g1 is None or np.array_equal(g1[i], blk["g1"]))
            for got, name in zip(tuple(basis) + tuple(experts), ("qa", "qb", "qc", "qd", "m_a", "m_Kq", "m_c", "m_d")):
                assert np.array_equal(got[i], blk[name]), name
        self.state_sets += 1
        return np.zeros(self.B, dtype=np.int32)

    def svi_run(self, K, iters, step_size, scale, batch_sizes, rows=None, seeds=None, resident_start=False):
        assert self.state_sets == 1 and seeds is None
        assert len(rows) == iters - (1 if resident_start else 0)
        self.runs.append((int(iters), len(rows), bool(resident_start)))
        trace = np.empty((iters, self.B))
        for it in range(iters):
            if not (resident_start and it == 0):
                sel = rows[it - (1 if resident_start else 0)]
                assert [len(r) for r in sel] == list(batch_sizes)
                self.batches.append([np.array(r) for r in sel])
                self.S = [self._subset(i, sel[i], m.canonical_expected()) for i, m in enumerate(self.shadow)]
            for i, m in enumerate(self.shadow):
                m._svi_step(self.S[i], float(scale[i]), step_size, False)
                _, sc = self.engs[i].estep(*m.canonical_expected())
                trace[it, i] = m._vlb_prior_terms() + sc[0]
        return trace, np.full(self.B, iters, dtype=np.int32), np.zeros(self.B, dtype=np.int32)

    svi_ilr_run = svi_run

    def vi_state(self, K):
        self.state_reads += 1
        blocks = [_gmm_blocks(m) for m in self.shadow]
        return {name: np.stack([blk[name] for blk in blocks]) for name in blocks[0]}

    def vi_ilr_state(self, K):
        self.state_reads += 1
        blocks = [fxi.model_blocks(m) for m in self.shadow]
        return {name: np.stack([blk[name] for blk in blocks]) for name in blocks[0]}


def _gmms(B):
    """B mixtures of the drivers fixture, two host iterations in (posterior != prior)."""
    g = load_golden("drivers_d3_k5_dir")
    engine = OracleEngine()
    models = [mc.build_gmm(g, engine)[1] for _ in range(B)]
    rng = np.random.default_rng(5)
    data = [g["X"], g["X"][:37] + 0.5, g["X"] + 0.1 * rng.standard_normal(g["X"].shape)][:B]
    npr.seed(9)
    meanfield_coordinate_descent_batched(models, data, randomize=True, maxiter=2, tol=0., sample_likelihood=False, engine=FakeResidentSvi())
    return models, data


def _batch(name):
    return _gmms(3) if name.startswith("drivers") else _ilrs(name, 3)


def _blocks_of(m):
    return (m.components,) if hasattr(m, "components") else (m.basis, m.models)


@pytest.mark.parametrize("name", ["ilr_dx1_dy1_k6_dir", "ilr_dx1_dy1_k50_stick", "drivers_d3_k5_dir"])
@pytest.mark.parametrize("maxiter,chunk,randomize,runs",
                         [(7, 3, False, [(3, 3, False), (3, 3, False), (1, 1, False)]),
                          (7, 3, True, [(3, 2, True), (3, 3, False), (1, 1, False)]),
                          (6, 8, True, [(6, 5, True)]), (4, 1, False, [(1, 1, False)] * 4), (4, 1, True, [(1, 0, True)] + [(1, 1, False)] * 3),
                          (0, 8, True, [])])
def test_driver_chunks_draws_and_writes_back_like_the_host_route(name, maxiter, chunk, randomize, runs):
    models, data = _batch(name)
    ref, _ = _batch(name)
    kw = dict(randomize=randomize, maxiter=maxiter, step_size=0.3, batch_size=16, sample_likelihood=False)
    fake = FakeResidentSvi(_batch(name)[0])
    npr.seed(3)
    random.seed(7)
    vlbs = meanfield_stochastic_descent_batched(models, data, engine=fake, resident=True, chunk=chunk, **kw)
    py_after = random.getstate()
    assert fake.runs == runs and [len(v) for v in vlbs] == [maxiter] * 3
    assert fake.prior_sets == fake.state_sets == fake.state_reads == (1 if maxiter else 0)
    host_fake = FakeResidentSvi()
    npr.seed(3)
    random.seed(7)
    host = meanfield_stochastic_descent_batched(ref, data, engine=host_fake, **kw)
    assert vlbs == host                                           # the same host step on both sides
    # the streams: Python's is consumed iteration by iteration and in model order, exactly as the host route consumes it; NumPy's
    # gave the same random start
    assert random.getstate() == py_after
    assert len(fake.batches) == len(host_fake.batches) == max(maxiter - (1 if randomize else 0), 0)
    for a, b in zip(fake.batches, host_fake.batches):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(fake.tables) == len(host_fake.tables) == (1 if randomize and maxiter else 0)
    for a, b in zip(fake.tables, host_fake.tables):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    gprior = mc.gating_of(load_golden(name), "gprior")[0]
    for m, r in zip(models, ref):
        for a, b in zip(np.atleast_2d(mc.gating_posterior(m.gating, gprior)), np.atleast_2d(mc.gating_posterior(r.gating, gprior))):
            assert np.array_equal(a, b)
        for bm, br in zip(_blocks_of(m), _blocks_of(r)):
            pm, pr = bm.posterior, br.posterior
            for a, b in zip(pm.params, pr.params):
                assert np.array_equal(a, b)
            for a, b in zip(pm.nat_param, pr.nat_param):
                assert np.array_equal(a, b)
            for a, b in zip(pm.expected_statistics(), pr.expected_statistics()):      # (the memos)
                assert np.array_equal(a, b)
            assert np.array_equal(pm._half_logdet_psi(), pr._half_logdet_psi())
        for a, b in zip(m.canonical_expected(), r.canonical_expected()):
            assert np.array_equal(a, b)
        assert m._vlb_prior_terms() == r._vlb_prior_terms()


def test_per_model_streams_and_philox_indices():
    """numpy_seeds / python_seeds: model i's draws run on its own streams under resident=True as on the host route, and the
    caller's generator states come back.  index_rng='philox': nothing is drawn from Python's generator, the seeds go to the
    engine, and the random start uses the iteration-0 indices of the device's stream."""
    from mimo_amd.mixtures.batched import philox_indices
    models, data = _gmms(3)
    ref, _ = _gmms(3)
    kw = dict(randomize=True, maxiter=5, step_size=0.3, batch_size=16, sample_likelihood=False, numpy_seeds=[5, 5, 6],
              python_seeds=[15, 15, 16])
    npstate, pystate = npr.get_state(), random.getstate()
    vlbs = meanfield_stochastic_descent_batched(models, data, engine=FakeResidentSvi(_gmms(3)[0]), resident=True, chunk=2, **kw)
    after = npr.get_state()
    assert np.array_equal(npstate[1], after[1]) and npstate[2:] == after[2:] and random.getstate() == pystate
    assert vlbs == meanfield_stochastic_descent_batched(ref, data, engine=FakeResidentSvi(), **kw)

    class Philox(FakeResidentSvi):
        def svi_run(self, K, iters, step_size, scale, batch_sizes, rows=None, seeds=None, resident_start=False):
            assert rows is None and list(seeds) == [21, 22, 23]
            self.runs.append((int(iters), 0, bool(resident_start)))
            return np.zeros((iters, self.B)), np.full(self.B, iters, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
    models, data = _gmms(3)
    fake = Philox(_gmms(3)[0])
    pystate = random.getstate()
    meanfield_stochastic_descent_batched(models, data, engine=fake, resident=True, chunk=4, index_rng='philox',
                                         seeds=[21, 22, 23], **dict(kw, python_seeds=None, batch_size=50))
    assert random.getstate() == pystate and fake.runs == [(4, 0, True), (1, 0, False)]
    for i, t in enumerate(fake.tables[0]):                             # (37 rows, 50 slots: rows drawn twice count twice)
        want = np.bincount(philox_indices(21 + i, t.shape[1], 50, 0), minlength=t.shape[1])
        assert np.allclose(t.sum(axis=0), want, rtol=0, atol=1e-12)
