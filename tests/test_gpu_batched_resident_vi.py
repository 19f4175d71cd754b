"""GPU: the device-resident batched VI (mimo_vi_prior_batched / mimo_vi_run_batched / mimo_vi_get_batched, mimo_vi_batched.hip) —
the update against 50-digit values with the host-native route as the yardstick, the operand image against the host packing rules
and the host-packed pass, batch independence, trace parity with the host route on plain and shared batches, stopping, chunking
and the refusals."""
import numpy as np
import pytest

import model_checks as mc
import vi_update_fixture as fx
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched

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


def _one_update(beng, shape):
    beng.upload(shape["rows"])
    S = beng.weighted_stats(shape["tables"])
    for b, s in enumerate(S):        # dyadic rows and weights: the device's statistics are the exact ones
        assert np.array_equal(s.n, shape["sn"][b]) and np.array_equal(s.sx, shape["sx"][b]) and np.array_equal(s.sxx, shape["sxx"][b])
    beng.vi_set_prior(**shape["prior"])
    trace, n_done, status = beng.vi_run(shape["K"], 1, 0.)
    assert not status.any() and list(n_done) == [1] * shape["B"] and np.all(np.isfinite(trace))
    return trace, beng.vi_state(shape["K"])


@pytest.mark.parametrize("idx", range(6))
def test_update_against_high_precision_with_the_host_route_as_yardstick(beng, idx):
    """err = max|x - hp| / max|hp| per (problem, component) block and output; err_device <= max(8 err_host, 2^-46), with the
    host-native route on the same inputs as the yardstick (factor 8: another elimination and summation order at equal precision
    over sums of at most 16 terms; floor: 64 ulp).  The two terms of the bound are exactly 0 where posterior = prior, so in the
    problem without rows, and there alone, their error is taken over the sum of the absolute values of their summands
    (vi_update_fixture.block_errors).
    Measured on the MI355X: the largest device error of a block is 1.25e-14 (E4 of one component at Dz = 3, K = 17, a value
    near zero after the digamma sum and log det cancel; the host route has the same bits and the same error), next 2.5e-15
    (E4 at Dz = 2, K = 4, host identical) and 2.1e-15 (bb at Dz = 16, host 2.2e-15); the largest device / host ratio of a
    block's maximum is 2.41 (c_total at Dz = 16: 5.4e-16 against 2.3e-16)."""
    shape = fx.shapes()[idx]
    _, state = _one_update(beng, shape)
    dev, host = fx.block_errors(state, shape), fx.block_errors(fx.host_state(shape), shape)
    bad = []
    for name in fx.BLOCKS:
        bound = np.maximum(8.0 * host[name], FLOOR)
        print(f"shape {idx} (B={shape['B']} Dz={shape['D']} K={shape['K']}) {name:9s} device {dev[name].max():.3e} "
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


@pytest.mark.parametrize("idx", [1, 3, 4])
def test_operand_image_is_the_host_packed_one(beng, idx):
    shape = fx.shapes()[idx]
    K, B = shape["K"], shape["B"]
    trace, state = _one_update(beng, shape)
    theta, S_loop, sc_loop = beng._vi_resident(K)
    for b in range(B):
        assert np.array_equal(theta[b], _pack(state["c_total"][b], state["bb"][b], state["W"][b])), b
        assert np.array_equal(state["W"][b], np.swapaxes(state["W"][b], 1, 2))
    # the pass saw what a host caller of estep(c, b, W) with those arrays sees
    S, sc = beng.estep(state["c_total"], state["bb"], state["W"])
    assert np.array_equal(sc[:, 0], sc_loop[:, 0])
    for a, l in zip(S, S_loop):
        assert np.array_equal(a.n, l.n) and np.array_equal(a.sx, l.sx) and np.array_equal(a.sxx, l.sxx)
    assert np.array_equal(trace[0], (state["vlb"][:, 0] + state["vlb"][:, 1]) + sc[:, 0])


def _problems(D, K, counts, seed):
    """Random problems with well-conditioned priors: rows, start tables, the priors as vi_set_prior takes them."""
    rng = np.random.default_rng(seed)
    B = len(counts)
    rows = [rng.standard_normal((n, D)) + 3.0 * rng.integers(-2, 3, size=(1, D)) for n in counts]
    tables = []
    for n in counts:
        r = rng.random((K, n))
        tables.append(r / r.sum(axis=0, keepdims=True))
    m0 = rng.standard_normal((B, K, D))
    kap = rng.uniform(0.05, 0.5, size=(B, K))
    G = rng.standard_normal((B, K, D, D)) / np.sqrt(D)
    P0 = np.eye(D) + G @ np.swapaxes(G, 2, 3)
    P0 = 0.5 * (P0 + np.swapaxes(P0, 2, 3))
    prior = dict(alpha0=rng.uniform(0.5, 2.0, size=(B, K)), pa=kap[..., None] * m0, pb=kap,
                 pc=P0 + kap[..., None, None] * (m0[..., :, None] * m0[..., None, :]), pd=np.full((B, K), 2.0),
                 prior_logZ=rng.standard_normal((B, K)))
    return rows, tables, prior


def _run(eng, rows, tables, prior, K, chunks, tol=0.):
    """upload, start, priors, vi_run per chunk -> (the traces stacked, n_done per chunk, the final state)."""
    eng.upload(rows)
    eng.weighted_stats(tables)
    eng.vi_set_prior(**prior)
    out = [eng.vi_run(K, n, tol) for n in chunks]
    assert not any(st.any() for _, _, st in out)
    return np.concatenate([t for t, _, _ in out]), [n for _, n, _ in out], eng.vi_state(K)


@pytest.mark.parametrize("D,K", [(2, 4), (16, 5), (3, 17)])
def test_a_problem_does_not_depend_on_its_batch(beng, D, K):
    rows, tables, prior = _problems(D, K, (40, 3, 77), seed=D * 100 + K)
    trace, _, state = _run(beng, rows, tables, prior, K, [3])
    assert np.all(np.isfinite(trace))
    for i in range(3):
        one = {k: v[i:i + 1] for k, v in prior.items()}
        t1, _, s1 = _run(beng, rows[i:i + 1], tables[i:i + 1], one, K, [3])
        assert np.array_equal(t1[:, 0], trace[:, i]), i
        assert _states_equal(state, s1, (i, 0)) is None, i


def _gmm_batch(engine, counts=(400, 37, 1200)):
    """B = 3 mixtures (Dz = 2, K = 4) on well-separated clusters, N_b = 400, 37, 1200 -> (build models, data)."""
    rng = np.random.default_rng(7)
    K, D = 4, 2
    centres = np.array([[-6., -6.], [-6., 6.], [6., -6.], [6., 6.]])
    data = [centres[rng.integers(0, K, size=n)] + 0.7 * rng.standard_normal((n, D)) + 0.3 * i for i, n in enumerate(counts)]
    g = dict(K=K, D=D, gating_kind="dirichlet", gprior_alphas=np.ones(K), prior_mus=np.zeros((K, D)), prior_kappas=0.01 * np.ones(K),
             prior_psis=np.stack([np.eye(D)] * K), prior_nus=(D + 2.) * np.ones(K))

    def build():
        return [mc.build_gmm(g, engine)[1] for _ in data]
    return build, data


def _block_err(a, b):
    """max|a - b| / max|b| per component block (leading axis K)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    K = a.shape[0]
    return np.max(np.abs(a - b).reshape(K, -1).max(axis=1) / np.abs(b).reshape(K, -1).max(axis=1))


def test_traces_equal_the_host_route(engine, beng):
    build, data = _gmm_batch(engine)
    kw = dict(randomize=True, init_rng='philox', seeds=[5, 6, 7], maxiter=6, tol=0., sample_likelihood=False, engine=beng)
    host_models, res_models = build(), build()
    host = meanfield_coordinate_descent_batched(host_models, data, **kw)
    res = meanfield_coordinate_descent_batched(res_models, data, resident=True, chunk=4, **kw)
    assert [len(v) for v in res] == [6, 6, 6] == [len(v) for v in host]
    for h, r in zip(host, res):
        assert np.all(np.abs(np.array(r) - np.array(h)) <= 1e-9 * np.abs(np.array(h))), (h, r)
    for hm, rm in zip(host_models, res_models):
        assert _block_err(rm.gating.posterior.alphas[:, None], hm.gating.posterior.alphas[:, None]) <= 1e-9
        for a, b in zip(rm.components.posterior.params, hm.components.posterior.params):
            assert _block_err(a, b) <= 1e-9
        for a, b in zip(rm.canonical_expected(), hm.canonical_expected()):       # the memo the write-back left
            assert _block_err(a, b) <= 1e-9
        assert abs(rm._vlb_prior_terms() - hm._vlb_prior_terms()) <= 1e-9 * abs(hm._vlb_prior_terms())


def test_shared_batch_equals_the_batch_of_copies(beng):
    D, K, B = 3, 17, 3
    rows, tables, prior = _problems(D, K, (150, 150, 150), seed=41)
    Z = rows[0]
    beng.upload([Z] * B)
    beng.weighted_stats(tables)
    beng.vi_set_prior(**prior)
    t_copies, n_copies, _ = beng.vi_run(K, 6, 0.)
    s_copies = beng.vi_state(K)
    beng.upload_shared(Z, B)
    beng.weighted_stats(tables)
    beng.vi_set_prior(**prior)
    t_shared, n_shared, st = beng.vi_run(K, 6, 0.)
    assert not st.any() and np.all(np.isfinite(t_shared))
    assert np.array_equal(t_shared, t_copies) and np.array_equal(n_shared, n_copies)
    assert _states_equal(s_copies, beng.vi_state(K)) is None


def test_stopping_follows_the_host_route(engine, beng):
    # small problems: from the random start each wanders for a different number of iterations (|delta vlb| of order 1 to 10) and
    # then settles within one or two (|delta vlb| < 1e-9) — on the large problems of the parity test the start is a long plateau
    build, data = _gmm_batch(engine, counts=(30, 45, 70))
    kw = dict(randomize=True, init_rng='philox', seeds=[5, 6, 7], sample_likelihood=False, engine=beng)
    full = meanfield_coordinate_descent_batched(build(), data, maxiter=28, tol=0., **kw)
    deltas = [np.abs(np.diff(np.array(v))) for v in full]
    # a tolerance at which the three problems stop at different iterations, every |delta vlb| up to its stop a factor >= 10 away
    tol = None
    for cand in 10.0 ** np.arange(0.0, -9.0, -0.25):
        stops = [int(np.argmax(d < cand)) if np.any(d < cand) else None for d in deltas]
        if None in stops or len(set(stops)) < 3:
            continue
        if all(np.all((d[:s + 1] >= 10.0 * cand) | (d[:s + 1] <= cand / 10.0)) for d, s in zip(deltas, stops)):
            tol = float(cand)
            break
    assert tol is not None, "no tolerance separates the three problems' stops by a factor 10: change the data of this test"
    host = meanfield_coordinate_descent_batched(build(), data, maxiter=28, tol=tol, **kw)
    lengths = [len(v) for v in host]
    assert len(set(lengths)) == 3 and max(lengths) < 28
    for v in host:                                         # the precondition, on the traces of the host route itself
        d = np.abs(np.diff(np.array(v)))
        assert np.all((d >= 10.0 * tol) | (d <= tol / 10.0))

    models = build()
    K = models[0].size
    from mimo_amd.distributions import native_sweep
    beng.upload([np.asarray(d, dtype=float) for d in data])
    beng.random_resp_stats(K, [5, 6, 7])
    blocks = [native_sweep._prior_block(m.components.prior) for m in models]
    beng.vi_set_prior(np.stack([m.gating.prior.alphas for m in models]), *(np.stack([blk[j] for blk in blocks]) for j in range(5)))
    done = np.zeros(3, dtype=int)
    frozen = [None] * 3
    for chunk in range(7):
        trace, n_done, status = beng.vi_run(K, 4, tol)
        assert not status.any()
        state = beng.vi_state(K)
        for i in range(3):
            assert np.all(np.isfinite(trace[:n_done[i], i])) and np.all(np.isnan(trace[n_done[i]:, i]))
            if frozen[i] is not None:                      # stopped in an earlier call: nothing appended, nothing moved
                assert n_done[i] == 0 and _states_equal(state, frozen[i], (i, i)) is None
            elif n_done[i] < 4 or done[i] + n_done[i] == lengths[i]:
                frozen[i] = state
        done += n_done
    assert list(done) == lengths
    assert all(f is not None for f in frozen)


def test_chunked_runs_equal_one_run(beng):
    D, K = 5, 20
    rows, tables, prior = _problems(D, K, (60, 200, 5), seed=9)
    t6, n6, s6 = _run(beng, rows, tables, prior, K, [6])
    t24, n24, s24 = _run(beng, rows, tables, prior, K, [2, 4])
    assert np.array_equal(t6, t24) and list(n6[0]) == [6, 6, 6] and [list(n) for n in n24] == [[2] * 3, [4] * 3]
    assert _states_equal(s6, s24) is None


def test_refusals(beng):
    D, K = 2, 4
    rows, tables, prior = _problems(D, K, (50, 20, 30), seed=3)
    eng = BatchedHipEngine(0)
    eng.upload(rows)
    eng.weighted_stats(tables)
    with pytest.raises(_lib.MimoHipError, match="prior"):            # before vi_set_prior
        eng.vi_run(K, 1, 0.)
    eng.vi_set_prior(**prior)
    eng.upload(rows)                                                 # an upload drops the priors and the statistics
    with pytest.raises(_lib.MimoHipError):
        eng.vi_run(K, 1, 0.)
    eng.weighted_stats(tables)
    eng.vi_set_prior(**prior)
    eng.estep(np.zeros((3, K)), np.zeros((3, K, D)), np.stack([np.stack([np.eye(D)] * K)] * 3), stats=False)
    with pytest.raises(_lib.MimoHipError, match="statistics"):       # the block was handed to a pass without statistics
        eng.vi_run(K, 1, 0.)
    eng.random_resp_stats(K + 1, [1, 2, 3])                          # a pass with another K
    with pytest.raises(_lib.MimoHipError, match="K = %d" % (K + 1)):
        eng.vi_run(K, 1, 0.)
    eng.weighted_stats(tables)
    eng.set_structure('diag')
    with pytest.raises(_lib.MimoHipError, match="full structure"):
        eng.vi_run(K, 1, 0.)
    eng.set_structure('full')
    t, n, st = eng.vi_run(K, 2, 0.)                                  # and the loop is still usable
    assert not st.any() and np.all(np.isfinite(t))
    # non-finite priors: refused by the engine before the library, and by the library itself
    for name in prior:
        bad = {k: v.copy() for k, v in prior.items()}
        bad[name].reshape(-1)[-1] = np.nan
        with pytest.raises(ValueError):
            eng.vi_set_prior(**bad)
        p = [np.ascontiguousarray(bad[k]) for k in ("alpha0", "pa", "pb", "pc", "pd", "prior_logZ")]
        assert eng._lib.mimo_vi_prior_batched(eng._ctx, K, *(v.ctypes.data for v in p)) == _lib.E_INVALID
    eng.close()


def test_an_indefinite_block_stops_its_problem_alone(engine, beng):
    D, K = 2, 4
    rows, tables, prior = _problems(D, K, (50, 20, 30), seed=3)
    bad = {k: v.copy() for k, v in prior.items()}
    bad["pc"][1, 2] = -1e4 * np.eye(D)                               # finite, and c - kappa m m' + statistics stays indefinite
    beng.upload(rows)
    beng.weighted_stats(tables)
    beng.vi_set_prior(**bad)
    before = beng.vi_state(K)
    trace, n_done, status = beng.vi_run(K, 3, 0.)
    assert list(status != 0) == [False, True, False] and list(n_done) == [3, 0, 3]
    assert np.all(np.isnan(trace[:, 1])) and np.all(np.isfinite(trace[:, [0, 2]]))
    state = beng.vi_state(K)
    assert _states_equal(state, before, (1, 1)) is None              # the failed problem's state is untouched
    t2, n2, st2 = beng.vi_run(K, 1, 0.)                              # ... and stays so
    assert list(n2) == [1, 0, 1] and st2[1] != 0 and _states_equal(beng.vi_state(K), before, (1, 1)) is None
    for i in (0, 2):                                                 # the other two: the numbers they have alone
        one = {k: v[i:i + 1] for k, v in prior.items()}
        t1, _, s1 = _run(beng, rows[i:i + 1], tables[i:i + 1], one, K, [3])
        assert np.array_equal(t1[:, 0], trace[:, i]) and _states_equal(state, s1, (i, 0)) is None

    # a block that fails at a LATER iteration: component 2 of problem 1 starts from a table that gives it huge weights (its block is
    # positive definite at the first update), the loop's own pass then leaves it the real, small statistics and the second
    # update fails; the problem keeps the state of its first iteration
    big = [t.copy() for t in tables]
    big[1][2] *= 1e6
    beng.upload(rows)
    beng.weighted_stats(big)
    beng.vi_set_prior(**bad)
    t1, n1, st1 = beng.vi_run(K, 1, 0.)
    assert not st1.any() and list(n1) == [1, 1, 1]
    first = beng.vi_state(K)
    t3, n3, st3 = beng.vi_run(K, 3, 0.)
    assert list(st3) == [0, 1, 0] and list(n3) == [3, 0, 3] and np.all(np.isnan(t3[:, 1])) and np.all(np.isfinite(t3[:, [0, 2]]))
    assert _states_equal(beng.vi_state(K), first, (1, 1)) is None and np.any(first["W"][1] != 0.)

    # a canonical form that is not finite without a bad pivot (nu = pd + n + Dz = 0.5 in a problem without rows: a digamma
    # argument below zero): status bit 2, nothing appended, the state untouched, the other problems alone as before
    nf = {k: v.copy() for k, v in prior.items()}
    nf["pd"][1] = -1.5
    beng.upload([rows[0], rows[1][:0], rows[2]])
    beng.weighted_stats([tables[0], tables[1][:, :0], tables[2]])
    beng.vi_set_prior(**nf)
    t4, n4, st4 = beng.vi_run(K, 2, 0.)
    assert list(st4) == [0, 2, 0] and list(n4) == [2, 0, 2] and np.all(np.isnan(t4[:, 1]))
    assert _states_equal(beng.vi_state(K), before, (1, 1)) is None
    assert np.array_equal(t4[:, [0, 2]], trace[:2][:, [0, 2]])

    # the driver raises what the NumPy route raises for such a block, naming the problem
    build, data = _gmm_batch(engine)
    models = build()
    from mimo_amd.distributions import native_sweep
    blk = native_sweep._prior_block(models[1].components.prior)
    pc = blk[2].copy()
    pc[0] = -1e6 * np.eye(2)
    models[1].components.prior._memo['sweep_c64'] = (blk[0], blk[1], pc, blk[3], blk[4])
    with pytest.raises(np.linalg.LinAlgError, match="problem 1"):
        meanfield_coordinate_descent_batched(models, data, randomize=True, init_rng='philox', seeds=[5, 6, 7], maxiter=4, tol=0.,
                                             sample_likelihood=False, engine=beng, resident=True)
