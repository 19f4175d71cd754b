"""GPU: the device-resident batched VI for mixtures of linear-Gaussian experts (mimo_vi_ilr_prior_batched / mimo_vi_ilr_run_batched /
mimo_vi_ilr_get_batched, mimo_vi_ilr_batched.hip) — the update against 50-digit values with the host route as the yardstick, the
operand image against the host packing rules and the host-packed pass, batch independence, trace parity with the host route,
stopping, chunking, the refusals and problems that fail alone."""
import numpy as np
import pytest

import vi_ilr_update_fixture as fx
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.distributions import (CategoricalWithDirichlet, CategoricalWithStickBreaking, Dirichlet, TruncatedStickBreaking,
                                    StackedNormalWisharts, StackedGaussiansWithNormalWisharts, StackedMatrixNormalWisharts,
                                    StackedLinearGaussiansWithMatrixNormalWisharts)
from mimo_amd.distributions import native_sweep
from mimo_amd.mixtures import BayesianMixtureOfLinearGaussians
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched, meanfield_coordinate_descent_batched_ilr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -46      # 64 ulp


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


def _states_equal(a, b, problems=None):
    for name in a:
        x, y = (a[name], b[name]) if problems is None else (a[name][problems[0]], b[name][problems[1]])
        if not np.array_equal(x, y):
            return name
    return None


def _set_prior(eng, prior):
    eng.vi_ilr_set_prior(prior["gating"], prior["g0"], prior["g1"], prior["basis"], prior["experts"])


def _one(prior, i):
    """Problem i's slice of a prior dict, as a batch of one."""
    return dict(gating=prior["gating"], g0=prior["g0"][i:i + 1], g1=None if prior["g1"] is None else prior["g1"][i:i + 1],
                basis=tuple(v[i:i + 1] for v in prior["basis"]), experts=tuple(v[i:i + 1] for v in prior["experts"]))


def _copy(prior):
    return dict(gating=prior["gating"], g0=prior["g0"].copy(), g1=None if prior["g1"] is None else prior["g1"].copy(),
                basis=tuple(v.copy() for v in prior["basis"]), experts=tuple(v.copy() for v in prior["experts"]))


def _one_update(beng, shape):
    beng.upload(shape["rows"])
    S = beng.weighted_stats(shape["tables"])
    for b, s in enumerate(S):        # dyadic rows and weights: the device's statistics are the exact ones
        assert np.array_equal(s.n, shape["sn"][b]) and np.array_equal(s.sx, shape["sz"][b]) and np.array_equal(s.sxx, shape["szz"][b])
    _set_prior(beng, shape["prior"])
    trace, n_done, status = beng.vi_ilr_run(shape["K"], 1, 0.)
    assert not status.any() and list(n_done) == [1] * shape["B"] and np.all(np.isfinite(trace))
    return trace, beng.vi_ilr_state(shape["K"])


@pytest.mark.parametrize("idx", range(8))
def test_update_against_high_precision_with_the_host_route_as_yardstick(beng, idx):
    """err = max|x - hp| / max|hp| per (problem, component) block and output; err_device <= max(8 err_host, 2^-46), with the
    host route on the same inputs as the yardstick (factor 8: another elimination and summation order at equal precision over
    sums of at most 16 terms; floor: 64 ulp).  The three terms of the bound are exactly 0 where posterior = prior, so in the
    problem without rows, and there alone, their error is taken over the sum of the absolute values of their summands
    (vi_ilr_update_fixture.block_errors).
    Measured on the MI355X: the largest device errors of a block are 1.25e-13 (hld of the basis at dx = dy = 1, K = 128, a value
    near zero; the host route has the same bits and the same error) and 1.19e-13 (m_E4 at dx = 15, dy = 1, host identical).
    Closest to the rule: a term of the bound at dx = 8, dy = 4, K = 5, device 1.37e-14 against host 2.26e-15, 0.96 of the bound
    (the 2^-46 floor); next 0.32 (a term at dx = 2, dy = 1, K = 17: 4.5e-15 against 3.6e-16) and 0.27.  Outside the terms of the
    bound the largest device / host ratio of a block's maximum is 3.3 (m_Kinv at dx = 1, dy = 3, K = 33: 5.8e-16 against
    1.8e-16)."""
    shape = fx.shapes()[idx]
    _, state = _one_update(beng, shape)
    dev, host = fx.block_errors(state, shape), fx.block_errors(fx.host_state(shape), shape)
    bad = []
    for name in fx.BLOCKS:
        bound = np.maximum(8.0 * host[name], FLOOR)
        print(f"shape {idx} (B={shape['B']} dx={shape['dx']} dy={shape['dy']} K={shape['K']}) {name:9s} device {dev[name].max():.3e} "
              f"host {host[name].max():.3e} worst device/bound {np.max(dev[name] / bound):.3f}")
        if not np.all(dev[name] <= bound):
            bad.append((name, float(dev[name].max()), float(host[name].max())))
    assert not bad, bad


def _pack(c, b, W):
    """The operand image of one problem from (c, b, W): the entry rules of the enumerator and the ThetaGeneric placement with
    RB = K16, NS = F16 / 4, identity order (mimo_theta.h), restated."""
    K, D = b.shape
    F = (D + 1) * (D + 2) // 2
    K16, NS = (K + 15) // 16, (F + 15) // 16 * 4
    img = np.zeros((K16, NS, 64))
    feat = lambda a, bb: a * (D + 1) - a * (a - 1) // 2 + (bb - a)

    def put(k, f, v):
        img[k // 16, f // 4, (f % 4) * 16 + k % 16] = v
    for k in range(K):
        put(k, feat(D, D), max(c[k], -1e300))
        for a in range(D):
            put(k, feat(a, D), b[k, a])
            put(k, feat(a, a), -0.5 * W[k, a, a])
            for bb in range(a + 1, D):
                put(k, feat(a, bb), -0.5 * (W[k, a, bb] + W[k, bb, a]))
    for k in range(K, 16 * K16):
        put(k, feat(D, D), -1e300)
    return img


@pytest.mark.parametrize("idx", [1, 3, 4, 6])
def test_operand_image_is_the_host_packed_one(beng, idx):
    shape = fx.shapes()[idx]
    K, B, dx = shape["K"], shape["B"], shape["dx"]
    trace, state = _one_update(beng, shape)
    theta, S_loop, sc_loop = beng._vi_resident(K)
    for b in range(B):
        assert np.array_equal(theta[b], _pack(state["c_total"][b], state["j_bb"][b], state["j_W"][b])), b
        assert np.array_equal(state["j_W"][b], np.swapaxes(state["j_W"][b], 1, 2))
        # the joint form is the sum embed_joint forms
        W = state["m_W"][b].copy()
        W[:, :dx, :dx] += state["W"][b]
        bb = state["m_bb"][b].copy()
        bb[:, :dx] += state["bb"][b]
        assert np.array_equal(W, state["j_W"][b]) and np.array_equal(bb, state["j_bb"][b])
        assert np.array_equal((state["cc"][b] + state["m_cc"][b]) + state["e_log_pi"][b], state["c_total"][b])
    # the pass saw what a host caller of estep(c, b, W) with those arrays sees
    S, sc = beng.estep(state["c_total"], state["j_bb"], state["j_W"])
    assert np.array_equal(sc[:, 0], sc_loop[:, 0])
    for a, l in zip(S, S_loop):
        assert np.array_equal(a.n, l.n) and np.array_equal(a.sx, l.sx) and np.array_equal(a.sxx, l.sxx)
    assert np.array_equal(trace[0], ((state["vlb"][:, 0] + state["vlb"][:, 1]) + state["vlb"][:, 2]) + sc[:, 0])


def _problems(dx, dy, K, counts, gating, seed):
    """Random problems with well-conditioned priors: rows, start tables, the priors as vi_ilr_set_prior takes them."""
    rng = np.random.default_rng(seed)
    B, D, dc = len(counts), dx + dy, dx + 1
    rows = [rng.standard_normal((n, D)) + 3.0 * rng.integers(-2, 3, size=(1, D)) for n in counts]
    tables = []
    for n in counts:
        r = rng.random((K, n))
        tables.append(r / r.sum(axis=0, keepdims=True))

    def spd(n):
        G = rng.standard_normal((B, K, n, n)) / np.sqrt(n)
        P = np.eye(n) + G @ np.swapaxes(G, 2, 3)
        return 0.5 * (P + np.swapaxes(P, 2, 3))
    m0 = rng.standard_normal((B, K, dx))
    kap = rng.uniform(0.05, 0.5, size=(B, K))
    basis = (kap[..., None] * m0, kap, spd(dx) + kap[..., None, None] * (m0[..., :, None] * m0[..., None, :]), np.full((B, K), 2.0),
             rng.standard_normal((B, K)))
    M0 = rng.standard_normal((B, K, dy, dc))
    K0 = spd(dc)
    ma = M0 @ K0
    mc = spd(dy) + ma @ np.swapaxes(M0, 2, 3)
    experts = (ma, K0, 0.5 * (mc + np.swapaxes(mc, 2, 3)), np.full((B, K), 1.0 + dc), rng.standard_normal((B, K)))
    stick = gating == 'stick-breaking'
    return rows, tables, dict(gating=gating, g0=rng.uniform(0.5, 2.0, size=(B, K)),
                              g1=rng.uniform(0.5, 4.0, size=(B, K)) if stick else None, basis=basis, experts=experts)


def _run(eng, rows, tables, prior, K, chunks, tol=0.):
    """upload, start, priors, vi_ilr_run per chunk -> (the traces stacked, n_done per chunk, the final state)."""
    eng.upload(rows)
    eng.weighted_stats(tables)
    _set_prior(eng, prior)
    out = [eng.vi_ilr_run(K, n, tol) for n in chunks]
    assert not any(st.any() for _, _, st in out)
    return np.concatenate([t for t, _, _ in out]), [n for _, n, _ in out], eng.vi_ilr_state(K)


CASES = [(1, 1, 6, 'dirichlet'), (2, 1, 17, 'stick-breaking'), (8, 4, 5, 'stick-breaking')]


@pytest.mark.parametrize("dx,dy,K,gating", CASES)
def test_a_problem_does_not_depend_on_its_batch(beng, dx, dy, K, gating):
    rows, tables, prior = _problems(dx, dy, K, (40, 3, 77), gating, seed=dx * 100 + K)
    trace, _, state = _run(beng, rows, tables, prior, K, [3])
    assert np.all(np.isfinite(trace))
    for i in range(3):
        t1, _, s1 = _run(beng, rows[i:i + 1], tables[i:i + 1], _one(prior, i), K, [3])
        assert np.array_equal(t1[:, 0], trace[:, i]), i
        assert _states_equal(state, s1, (i, 0)) is None, i


def test_shared_batch_equals_the_batch_of_copies(beng):
    dx, dy, K, B = 2, 1, 17, 3
    rows, tables, prior = _problems(dx, dy, K, (150, 150, 150), 'stick-breaking', seed=41)
    Z = rows[0]
    beng.upload([Z] * B)
    beng.weighted_stats(tables)
    _set_prior(beng, prior)
    t_copies, n_copies, _ = beng.vi_ilr_run(K, 6, 0.)
    s_copies = beng.vi_ilr_state(K)
    beng.upload_shared(Z, B)
    beng.weighted_stats(tables)
    _set_prior(beng, prior)
    t_shared, n_shared, st = beng.vi_ilr_run(K, 6, 0.)
    assert not st.any() and np.all(np.isfinite(t_shared))
    assert np.array_equal(t_shared, t_copies) and np.array_equal(n_shared, n_copies)
    assert _states_equal(s_copies, beng.vi_ilr_state(K)) is None


def test_chunked_runs_equal_one_run(beng):
    dx, dy, K = 3, 2, 20
    rows, tables, prior = _problems(dx, dy, K, (60, 200, 5), 'dirichlet', seed=9)
    t6, n6, s6 = _run(beng, rows, tables, prior, K, [6])
    t24, n24, s24 = _run(beng, rows, tables, prior, K, [2, 4])
    assert np.array_equal(t6, t24) and list(n6[0]) == [6, 6, 6] and [list(n) for n in n24] == [[2] * 3, [4] * 3]
    assert _states_equal(s6, s24) is None


def _ilr_batch(engine, dx, K, gating, counts, seed=7):
    """B synthetic piecewise-linear regression problems (dy = 1) -> (build models, data)."""
    rng = np.random.default_rng(seed)
    dy, dc = 1, dx + 1
    knots = np.linspace(-3.0, 3.0, 5)
    slopes = np.array([2.0, -1.0, 0.5, -2.5, 1.5, 3.0])
    data = []
    for i, n in enumerate(counts):
        x = rng.uniform(-3.0, 3.0, size=(n, dx))
        seg = np.searchsorted(knots, x[:, 0])
        y = slopes[seg] * x[:, 0] + 0.5 * seg + 0.3 * x[:, 1:].sum(axis=1) + 0.2 * rng.standard_normal(n) + 0.3 * i
        data.append((x, y[:, None]))

    def build():
        models = []
        for _ in counts:
            if gating == 'dirichlet':
                gate = CategoricalWithDirichlet(dim=K, prior=Dirichlet(dim=K, alphas=np.ones(K)))
            else:
                gate = CategoricalWithStickBreaking(dim=K, prior=TruncatedStickBreaking(dim=K, gammas=np.ones(K), deltas=5.0 * np.ones(K)))
            bprior = StackedNormalWisharts(size=K, dim=dx, mus=np.zeros((K, dx)), kappas=0.01 * np.ones(K),
                                           psis=np.stack([np.eye(dx)] * K), nus=(dx + 2.) * np.ones(K))
            mprior = StackedMatrixNormalWisharts(K, dc, dy, Ms=np.zeros((K, dy, dc)), Ks=np.stack([0.01 * np.eye(dc)] * K),
                                                 psis=np.stack([np.eye(dy)] * K), nus=(dy + 2.) * np.ones(K))
            models.append(BayesianMixtureOfLinearGaussians(
                size=K, input_dim=dx, output_dim=dy, gating=gate,
                basis=StackedGaussiansWithNormalWisharts(size=K, dim=dx, prior=bprior, engine=engine),
                models=StackedLinearGaussiansWithMatrixNormalWisharts(K, dc, dy, mprior, affine=True, engine=engine), engine=engine))
        return models
    return build, data


def _block_err(a, b):
    """max|a - b| / max|b| per component block (leading axis K)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    K = a.shape[0]
    return np.max(np.abs(a - b).reshape(K, -1).max(axis=1) / np.abs(b).reshape(K, -1).max(axis=1))


def _gating_params(model):
    p = model.gating.posterior
    return (p.alphas,) if isinstance(p, Dirichlet) else (p.gammas, p.deltas)


@pytest.mark.parametrize("dx,K,gating", [(1, 6, 'dirichlet'), (2, 17, 'stick-breaking')])
def test_traces_equal_the_host_route(engine, beng, dx, K, gating):
    build, data = _ilr_batch(engine, dx, K, gating, (400, 37, 1200))
    kw = dict(randomize=True, init_rng='philox', seeds=[5, 6, 7], maxiter=6, tol=0., engine=beng)
    host_models, res_models = build(), build()
    host = meanfield_coordinate_descent_batched(host_models, data, sample_likelihood=False, **kw)
    res = meanfield_coordinate_descent_batched_ilr(res_models, data, chunk=4, **kw)
    assert [len(v) for v in res] == [6, 6, 6] == [len(v) for v in host]
    for h, r in zip(host, res):
        print("host", h, "resident", r)
        assert np.all(np.abs(np.array(r) - np.array(h)) <= 1e-9 * np.abs(np.array(h))), (h, r)
    for hm, rm in zip(host_models, res_models):
        for a, b in zip(_gating_params(rm), _gating_params(hm)):
            assert _block_err(a[:, None], b[:, None]) <= 1e-9
        for blk in ("basis", "models"):
            for a, b in zip(getattr(rm, blk).posterior.params, getattr(hm, blk).posterior.params):
                assert _block_err(a, b) <= 1e-9, blk
        for a, b in zip(rm.canonical_expected(), hm.canonical_expected()):       # the memos the write-back left
            assert _block_err(a, b) <= 1e-9
        assert abs(rm._vlb_prior_terms() - hm._vlb_prior_terms()) <= 1e-9 * abs(hm._vlb_prior_terms())


def _model_priors(models):
    stick = isinstance(models[0].gating.prior, TruncatedStickBreaking)
    bb = [native_sweep._prior_block(m.basis.prior) for m in models]
    mb = [native_sweep._prior_block(m.models.prior) for m in models]
    return dict(gating='stick-breaking' if stick else 'dirichlet',
                g0=np.stack([np.asarray(m.gating.prior.gammas if stick else m.gating.prior.alphas, dtype=float) for m in models]),
                g1=np.stack([np.asarray(m.gating.prior.deltas, dtype=float) for m in models]) if stick else None,
                basis=tuple(np.stack([b[j] for b in bb]) for j in range(5)), experts=tuple(np.stack([b[j] for b in mb]) for j in range(5)))


def test_stopping_follows_the_host_route(engine, beng):
    # An ILR trace decays smoothly, so a tolerance with a factor 10 of room on both sides of every stop is rare: this data set
    # (found on the CPU oracle) has one near 1.8e-2, where the three problems stop after 13, 17 and 32 iterations.  The start is
    # the host-drawn one, the same table on both routes.
    import numpy.random as npr
    maxiter, seed = 60, 11
    build, data = _ilr_batch(engine, 1, 6, 'dirichlet', (20, 60, 150), seed=11)
    kw = dict(randomize=True, init_rng='host', sample_likelihood=False, engine=beng)
    npr.seed(seed)
    full = meanfield_coordinate_descent_batched(build(), data, maxiter=maxiter, tol=0., **kw)
    deltas = [np.abs(np.diff(np.array(v))) for v in full]
    # a tolerance at which the three problems stop at different iterations, every |delta vlb| up to its stop a factor >= 10 away
    found = None
    for cand in 10.0 ** np.arange(0.0, -9.0, -0.25):
        stops = [int(np.argmax(d < cand)) if np.any(d < cand) else None for d in deltas]
        if None in stops or len(set(stops)) < 3:
            continue
        if all(np.all((d[:s + 1] >= 10.0 * cand) | (d[:s + 1] <= cand / 10.0)) for d, s in zip(deltas, stops)):
            found = float(cand)
            break
    assert found is not None, "no tolerance separates the three problems' stops by a factor 10: change the data of this test"
    tol = found
    npr.seed(seed)
    host = meanfield_coordinate_descent_batched(build(), data, maxiter=maxiter, tol=tol, **kw)
    lengths = [len(v) for v in host]
    assert len(set(lengths)) == 3 and max(lengths) < maxiter
    for v in host:                                         # the precondition, on the traces of the host route itself
        d = np.abs(np.diff(np.array(v)))
        assert np.all((d >= 10.0 * tol) | (d <= tol / 10.0))

    npr.seed(seed)
    models = build()                                       # (the constructors draw, as in the two calls above)
    K = models[0].size
    beng.upload([np.hstack([x, y]) for x, y in data])
    tables = []
    for x, _ in data:                                      # the host start of the drivers (_random_start)
        r = npr.rand(K, len(x))
        tables.append(r / np.sum(r, axis=0))
    beng.weighted_stats(tables)
    _set_prior(beng, _model_priors(models))
    done = np.zeros(3, dtype=int)
    frozen = [None] * 3
    for chunk in range(maxiter // 4):
        trace, n_done, status = beng.vi_ilr_run(K, 4, tol)
        assert not status.any()
        state = beng.vi_ilr_state(K)
        for i in range(3):
            assert np.all(np.isfinite(trace[:n_done[i], i])) and np.all(np.isnan(trace[n_done[i]:, i]))
            if frozen[i] is not None:                      # stopped in an earlier call: nothing appended, nothing moved
                assert n_done[i] == 0 and _states_equal(state, frozen[i], (i, i)) is None
            elif n_done[i] < 4 or done[i] + n_done[i] == lengths[i]:
                frozen[i] = state
        done += n_done
    assert list(done) == lengths
    assert all(f is not None for f in frozen)


def test_refusals(beng):
    dx, dy, K = 1, 1, 4
    D = dx + dy
    rows, tables, prior = _problems(dx, dy, K, (50, 20, 30), 'stick-breaking', seed=3)
    eng = BatchedHipEngine(0)
    eng.upload(rows)
    eng.weighted_stats(tables)
    with pytest.raises(_lib.MimoHipError, match="prior"):            # before vi_ilr_set_prior
        eng.vi_ilr_run(K, 1, 0.)
    _set_prior(eng, prior)
    eng.upload(rows)                                                 # an upload drops the priors and the statistics
    with pytest.raises(_lib.MimoHipError, match="prior"):
        eng.vi_ilr_run(K, 1, 0.)
    eng.weighted_stats(tables)
    _set_prior(eng, prior)
    eng.estep(np.zeros((3, K)), np.zeros((3, K, D)), np.stack([np.stack([np.eye(D)] * K)] * 3), stats=False)
    with pytest.raises(_lib.MimoHipError, match="statistics"):       # the block was handed to a pass without statistics
        eng.vi_ilr_run(K, 1, 0.)
    eng.random_resp_stats(K + 1, [1, 2, 3])                          # a pass with another K
    with pytest.raises(_lib.MimoHipError, match="K = %d" % (K + 1)):
        eng.vi_ilr_run(K, 1, 0.)
    eng.weighted_stats(tables)
    eng.set_structure('diag')
    with pytest.raises(_lib.MimoHipError, match="full structure"):
        eng.vi_ilr_run(K, 1, 0.)
    eng.set_structure('full')
    t, n, st = eng.vi_ilr_run(K, 2, 0.)                              # and the loop is still usable
    assert not st.any() and np.all(np.isfinite(t))
    # dx + dy != Dz: refused by the engine before the library, and by the library itself
    _, _, wide = _problems(2, 1, K, (50, 20, 30), 'stick-breaking', seed=3)
    with pytest.raises(ValueError, match="Dz"):
        _set_prior(eng, wide)
    flat = lambda pr: [np.ascontiguousarray(v) for v in (pr["g0"], pr["g1"]) + tuple(pr["basis"]) + tuple(pr["experts"])]
    assert eng._lib.mimo_vi_ilr_prior_batched(eng._ctx, K, 2, 1, 1, *(v.ctypes.data for v in flat(wide))) == _lib.E_INVALID
    assert eng._lib.mimo_vi_ilr_prior_batched(eng._ctx, K, dx, dy, 7, *(v.ctypes.data for v in flat(prior))) == _lib.E_INVALID
    # non-finite priors: refused by the engine before the library, and by the library itself
    for pos in range(12):
        bad = _copy(prior)
        flat(bad)[pos].reshape(-1)[-1] = np.nan
        with pytest.raises(ValueError):
            _set_prior(eng, bad)
        assert eng._lib.mimo_vi_ilr_prior_batched(eng._ctx, K, dx, dy, 1, *(v.ctypes.data for v in flat(bad))) == _lib.E_INVALID
    # (a refused prior call leaves the loop as it was)
    t, n, st = eng.vi_ilr_run(K, 1, 0.)
    assert not st.any() and np.all(np.isfinite(t))

    # one family at a time: each loop refuses the other's prior block and names the families; the test hook serves both
    with pytest.raises(_lib.MimoHipError, match="that of mixtures of linear-Gaussian experts"):
        eng.vi_run(K, 1, 0.)
    with pytest.raises(_lib.MimoHipError, match="that of mixtures of linear-Gaussian experts"):
        eng.vi_state(K)
    theta, _, _ = eng._vi_resident(K)
    assert np.any(theta != 0.)
    rng = np.random.default_rng(1)
    gmm = dict(alpha0=np.ones((3, K)), pa=np.zeros((3, K, D)), pb=np.full((3, K), 0.1), pc=np.stack([np.stack([np.eye(D)] * K)] * 3),
               pd=np.full((3, K), 2.0), prior_logZ=rng.standard_normal((3, K)))
    eng.weighted_stats(tables)
    eng.vi_set_prior(**gmm)
    with pytest.raises(_lib.MimoHipError, match="that of mixtures of Gaussians"):
        eng.vi_ilr_run(K, 1, 0.)
    with pytest.raises(_lib.MimoHipError, match="that of mixtures of Gaussians"):
        eng.vi_ilr_state(K)
    t, n, st = eng.vi_run(K, 1, 0.)                                  # the GMM loop runs on its own prior
    assert not st.any() and np.all(np.isfinite(t))
    eng._vi_resident(K)
    _set_prior(eng, prior)                                           # ... and the ILR loop again on its own
    t, n, st = eng.vi_ilr_run(K, 1, 0.)
    assert not st.any() and np.all(np.isfinite(t))
    eng.close()


def _fails_alone(beng, rows, tables, prior, bad, K, bit, iters=3):
    beng.upload(rows)
    beng.weighted_stats(tables)
    _set_prior(beng, bad)
    before = beng.vi_ilr_state(K)
    trace, n_done, status = beng.vi_ilr_run(K, iters, 0.)
    assert list(status) == [0, bit, 0] and list(n_done) == [iters, 0, iters]
    assert np.all(np.isnan(trace[:, 1])) and np.all(np.isfinite(trace[:, [0, 2]]))
    state = beng.vi_ilr_state(K)
    assert _states_equal(state, before, (1, 1)) is None              # the failed problem's state is untouched
    t2, n2, st2 = beng.vi_ilr_run(K, 1, 0.)                          # ... and stays so
    assert list(n2) == [1, 0, 1] and st2[1] == bit and _states_equal(beng.vi_ilr_state(K), before, (1, 1)) is None
    for i in (0, 2):                                                 # the other two: the numbers they have alone
        t1, _, s1 = _run(beng, rows[i:i + 1], tables[i:i + 1], _one(prior, i), K, [iters])
        assert np.array_equal(t1[:, 0], trace[:, i]) and _states_equal(state, s1, (i, 0)) is None


@pytest.mark.parametrize("which", ["experts_c", "experts_K", "basis_c"])
def test_an_indefinite_block_stops_its_problem_alone(beng, which):
    """Ordinary finite inputs: a prior block so negative that the posterior block stays indefinite with the statistics added."""
    dx, dy, K = 2, 2, 4
    rows, tables, prior = _problems(dx, dy, K, (50, 20, 30), 'dirichlet', seed=3)
    bad = _copy(prior)
    if which == "experts_c":
        bad["experts"][2][1, 2] = -1e4 * np.eye(dy)
    elif which == "experts_K":
        bad["experts"][1][1, 2] = -1e4 * np.eye(dx + 1)
    else:
        bad["basis"][2][1, 2] = -1e4 * np.eye(dx)
    _fails_alone(beng, rows, tables, prior, bad, K, 1)


def test_a_non_finite_form_stops_its_problem_alone(beng):
    """nu = md + dy + 1 - dc = -1.5 in a problem without rows: a digamma argument below zero, no bad pivot — status bit 2."""
    dx, dy, K = 1, 1, 4
    rows, tables, prior = _problems(dx, dy, K, (50, 20, 30), 'stick-breaking', seed=5)
    rows[1], tables[1] = rows[1][:0], tables[1][:, :0]
    bad = _copy(prior)
    bad["experts"][3][1] = -1.5
    _fails_alone(beng, rows, tables, prior, bad, K, 2, iters=2)


def test_the_driver_names_the_failing_problem(engine, beng):
    build, data = _ilr_batch(engine, 1, 6, 'dirichlet', (400, 37, 1200))
    kw = dict(randomize=True, init_rng='philox', seeds=[5, 6, 7], maxiter=4, tol=0., engine=beng)
    models = build()
    blk = native_sweep._prior_block(models[1].models.prior)
    mc_ = blk[2].copy()
    mc_[0] = -1e6 * np.eye(1)
    models[1].models.prior._memo['sweep_c64'] = (blk[0], blk[1], mc_, blk[3], blk[4])
    with pytest.raises(np.linalg.LinAlgError, match="problem 1"):
        meanfield_coordinate_descent_batched_ilr(models, data, **kw)
    models = build()
    blk = native_sweep._prior_block(models[2].models.prior)
    models[2].models.prior._memo['sweep_c64'] = (blk[0], blk[1], blk[2], np.full_like(blk[3], -1e6), blk[4])
    with pytest.raises(FloatingPointError, match="problem 2"):
        meanfield_coordinate_descent_batched_ilr(models, data, **kw)


NW_PARTS = ('qa', 'qb', 'qc', 'qd', 'mus', 'psis', 'nus', 'hld', 'cc', 'bb', 'W', 'E2', 'E4')


@pytest.mark.parametrize("gating", ['dirichlet', 'stick-breaking'])
@pytest.mark.parametrize("dx,dy,K", [(1, 1, 128), (1, 15, 17), (15, 1, 5), (8, 4, 33)])
def test_the_basis_block_is_the_gmm_loops_normal_wishart_block(beng, dx, dy, K, gating):
    """The ILR loop's basis parts are the GMM loop's Normal-Wishart parts on the x columns, bit for bit, in all three modes: one
    conjugate iteration, an uploaded posterior (init) and one SVI step on the resident statistics (blend).  Dyadic rows and
    tables: the statistics of x are exactly the x block of the statistics of z, whatever the order of the sums."""
    counts = (9, 0, 12)          # (one problem without rows)
    B = len(counts)
    _, _, prior = _problems(dx, dy, K, (4, 4, 4), gating, seed=100 * dx + dy)
    rng = np.random.default_rng(K)
    rows = [rng.integers(-16, 17, size=(n, dx + dy)) / 8.0 for n in counts]
    tables = [rng.integers(0, 17, size=(K, n)) / 16.0 for n in counts]
    pa, pb, pc, pd, plz = prior["basis"]
    gmm_prior = dict(alpha0=prior["g0"], pa=pa, pb=pb, pc=pc, pd=pd, prior_logZ=plz)
    half, none = np.full(B, 0.5), np.zeros(B, dtype=np.int64)

    def exact(z):
        S = beng.weighted_stats(tables)
        for b, s in enumerate(S):
            assert np.array_equal(s.n, tables[b].sum(axis=1)) and np.array_equal(s.sx, tables[b] @ z[b]) \
                and np.array_equal(s.sxx, np.einsum('kn,na,nb->kab', tables[b], z[b], z[b]))

    def ok(out):
        assert not out[-1].any()

    # mixtures of linear-Gaussian experts over z = [x, y]
    beng.upload(rows)
    exact(rows)
    _set_prior(beng, prior)
    ok(beng.vi_ilr_run(K, 1, 0.))
    ilr = [beng.vi_ilr_state(K)]
    exact(rows)
    s = ilr[0]
    assert not beng.svi_ilr_set_state(s['g0'], s['g1'] if gating == 'stick-breaking' else None, tuple(s[n] for n in NW_PARTS[:4]),
                                      (s['m_a'], s['m_Kq'], s['m_c'], s['m_d'])).any()
    ilr.append(beng.vi_ilr_state(K))
    ok(beng.svi_ilr_run(K, 1, 0.5, half, none, rows=[], resident_start=True))
    ilr.append(beng.vi_ilr_state(K))

    # mixtures of Gaussians over x alone, the basis prior as the components' prior
    xs = [np.ascontiguousarray(z[:, :dx]) for z in rows]
    beng.upload(xs)
    exact(xs)
    beng.vi_set_prior(**gmm_prior)
    ok(beng.vi_run(K, 1, 0.))
    gmm = [beng.vi_state(K)]
    exact(xs)
    assert not beng.svi_set_state(gmm[0]['alpha'], *(s[n] for n in NW_PARTS[:4])).any()
    gmm.append(beng.vi_state(K))
    ok(beng.svi_run(K, 1, 0.5, half, none, rows=[], resident_start=True))
    gmm.append(beng.vi_state(K))

    for mode, a, g in zip(('conjugate', 'init', 'blend'), ilr, gmm):
        for name in NW_PARTS:
            assert np.array_equal(a[name], g[name]), (mode, name)
