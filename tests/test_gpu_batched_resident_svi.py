"""GPU: the device-resident batched SVI (mimo_svi_state_batched / mimo_svi_run_batched and their _ilr_ forms; the blend and init
modes of mimo_vi_batched.hip / mimo_vi_ilr_batched.hip, svi_indices_kernel) — step size 1 against the conjugate loop bit for bit,
the blend against the NumPy expression of the host step bit for bit, the driver against the host route at the fixtures' own
tolerances, batch independence and chunking, the device's index draws against their host mirror, failures and refusals."""
import numpy as np
import pytest

import test_gpu_batched_resident_ilr as ti
import test_gpu_batched_resident_vi as tg
from conftest import rel_err
from test_gpu_batched_svi import CASES as HOST_CASES, NUMPY_SEEDS, PYTHON_SEEDS, _models, _posterior, _refuse
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.distributions import native_sweep
from mimo_amd.distributions.bayesian import stick_acc_counts
from mimo_amd.engine import HipEngine, philox_uniforms
from mimo_amd.mixtures.batched import (_ilr_resident_reason, meanfield_stochastic_descent_batched, philox_indices)

pytestmark = pytest.mark.gpu

COUNTS = (40, 64, 200)


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


class Gmm:
    """One family behind the names the tests use: problems, priors, the loop's calls, the natural parameters of a state."""
    NAT = ('alpha', 'qa', 'qb', 'qc', 'qd')

    def __init__(self, D, K):
        self.D, self.K, self.id = D, K, f"gmm-{D}-{K}"

    def problems(self, counts, seed):
        return tg._problems(self.D, self.K, counts, seed)

    def set_prior(self, eng, prior):
        eng.vi_set_prior(**prior)

    def one(self, prior, i):
        return {k: v[i:i + 1] for k, v in prior.items()}

    def prior_of(self, prior, b):
        return {k: v[b] for k, v in prior.items()}

    def vi_run(self, eng, n):
        return eng.vi_run(self.K, n, 0.)

    def state(self, eng):
        return eng.vi_state(self.K)

    def set_state(self, eng, st):
        return eng.svi_set_state(*(st[name] for name in self.NAT))

    def svi_run(self, eng, *a, **kw):
        return eng.svi_run(self.K, *a, **kw)

    def prior_as_state(self, prior):
        return dict(alpha=prior["alpha0"], qa=prior["pa"], qb=prior["pb"], qc=prior["pc"], qd=prior["pd"])

    def image(self, st, b):
        return tg._pack(st["c_total"][b], st["bb"][b], st["W"][b])

    def host_blend(self, prior, cur, S, rho, scale):
        """The NumPy expressions of _ConjugateBlock._apply_sgd and CategoricalWithDirichlet.meanfield_sgd on problem b's parts."""
        blend = lambda c, p, s: (1. - rho) * c + rho * (p + 1. / scale * s)
        out = dict(qa=blend(cur["qa"], prior["pa"], S.sx), qb=blend(cur["qb"], prior["pb"], S.n),
                   qc=blend(cur["qc"], prior["pc"], S.sxx), qd=blend(cur["qd"], prior["pd"], S.n))
        out["alpha"] = blend(cur["alpha"] - 1., prior["alpha0"] - 1., S.n) + 1.
        return out


class Ilr:
    NAT = ('g0', 'g1', 'qa', 'qb', 'qc', 'qd', 'm_a', 'm_Kq', 'm_c', 'm_d')

    def __init__(self, dx, dy, K, gating):
        self.dx, self.dy, self.K, self.gating, self.id = dx, dy, K, gating, f"ilr-{dx}-{dy}-{K}-{gating}"
        self.stick = gating == 'stick-breaking'

    def problems(self, counts, seed):
        return ti._problems(self.dx, self.dy, self.K, counts, self.gating, seed)

    def set_prior(self, eng, prior):
        ti._set_prior(eng, prior)

    def one(self, prior, i):
        return ti._one(prior, i)

    def prior_of(self, prior, b):
        return dict(g0=prior["g0"][b], g1=None if prior["g1"] is None else prior["g1"][b], basis=[v[b] for v in prior["basis"]],
                    experts=[v[b] for v in prior["experts"]])

    def vi_run(self, eng, n):
        return eng.vi_ilr_run(self.K, n, 0.)

    def state(self, eng):
        return eng.vi_ilr_state(self.K)

    def set_state(self, eng, st):
        return eng.svi_ilr_set_state(st['g0'], st['g1'] if self.stick else None, [st[n] for n in ('qa', 'qb', 'qc', 'qd')],
                                     [st[n] for n in ('m_a', 'm_Kq', 'm_c', 'm_d')])

    def svi_run(self, eng, *a, **kw):
        return eng.svi_ilr_run(self.K, *a, **kw)

    def prior_as_state(self, prior):
        st = dict(g0=prior["g0"], g1=prior["g1"] if self.stick else np.zeros_like(prior["g0"]))
        st.update(zip(('qa', 'qb', 'qc', 'qd'), prior["basis"][:4]))
        st.update(zip(('m_a', 'm_Kq', 'm_c', 'm_d'), prior["experts"][:4]))
        return st

    def image(self, st, b):
        return ti._pack(st["c_total"][b], st["j_bb"][b], st["j_W"][b])

    def host_blend(self, prior, cur, S, rho, scale):
        """The NumPy expressions of _apply_sgd on the basis and the experts (statistics cut as split_joint_stats cuts them)
        and of the two gatings' meanfield_sgd, on problem b's parts."""
        dx = self.dx
        blend = lambda c, p, s: (1. - rho) * c + rho * (p + 1. / scale * s)
        n, sz, szz = S.n, S.sx, S.sxx
        K = len(n)
        yxt = np.concatenate([szz[:, dx:, :dx], sz[:, dx:, None]], axis=2)
        xtxt = np.zeros((K, dx + 1, dx + 1))
        xtxt[:, :dx, :dx], xtxt[:, :dx, dx], xtxt[:, dx, :dx], xtxt[:, dx, dx] = szz[:, :dx, :dx], sz[:, :dx], sz[:, :dx], n
        pa, pb, pc, pd = prior["basis"][:4]
        ma, mb, mc_, md = prior["experts"][:4]
        out = dict(qa=blend(cur["qa"], pa, sz[:, :dx]), qb=blend(cur["qb"], pb, n), qc=blend(cur["qc"], pc, szz[:, :dx, :dx]),
                   qd=blend(cur["qd"], pd, n), m_a=blend(cur["m_a"], ma, yxt), m_Kq=blend(cur["m_Kq"], mb, xtxt),
                   m_c=blend(cur["m_c"], mc_, szz[:, dx:, dx:]), m_d=blend(cur["m_d"], md, n))
        if self.stick:
            out["g0"] = blend(cur["g0"], prior["g0"], n)
            out["g1"] = blend(cur["g1"], prior["g1"], stick_acc_counts(n))
        else:
            out["g0"] = blend(cur["g0"] - 1., prior["g0"] - 1., n) + 1.
            out["g1"] = np.zeros(K)
        return out


FAMILIES = [Gmm(2, 4), Gmm(3, 17), Gmm(16, 5), Ilr(1, 1, 6, 'dirichlet'), Ilr(2, 1, 17, 'stick-breaking'), Ilr(8, 4, 5, 'dirichlet')]
DEEP = Ilr(1, 1, 128, 'stick-breaking')      # (the descending sum over 127 later sticks)
ids = lambda fams: [f.id for f in fams]


def _start(eng, fam, rows, tables, prior, state=None):
    """upload, the start's statistics, priors, a starting posterior (default: the prior itself) -> the init status."""
    eng.upload(rows)
    eng.weighted_stats(tables)
    fam.set_prior(eng, prior)
    return fam.set_state(eng, fam.prior_as_state(prior) if state is None else state)


def _posterior_state(eng, fam, rows, tables, prior):
    """A posterior that is not the prior: the state after one conjugate iteration from `tables`."""
    eng.upload(rows)
    eng.weighted_stats(tables)
    fam.set_prior(eng, prior)
    _, _, st = fam.vi_run(eng, 1)
    assert not st.any()
    return fam.state(eng)


def _draws(counts, sizes, n, seed):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, c, size=s) for c, s in zip(counts, sizes)] for _ in range(n)]


# ---- 1. step size 1 is the conjugate loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES + [DEEP], ids=ids(FAMILIES + [DEEP]))
def test_step_size_one_is_the_conjugate_loop_bit_for_bit(beng, fam):
    """(1 - 1) eta = 0 and 1 (eta0 + 1 S) = eta0 + S exactly, and the identity selection is the plain pass: svi_run(3) from the
    start's statistics equals vi_run(3) in trace, posterior blocks, operand images and the last pass's scalars.  The statistics
    svi_run leaves are those of its last minibatch pass, which ran on the image of iteration 2: vi_run's after two iterations."""
    counts = COUNTS if fam is not DEEP else (40, 64)
    rows, tables, prior = fam.problems(counts, seed=11)
    B = len(counts)
    beng.upload(rows)
    beng.weighted_stats(tables)
    fam.set_prior(beng, prior)
    t2, _, st = fam.vi_run(beng, 2)
    _, S2, _ = beng._vi_resident(fam.K)
    t1, _, st1 = fam.vi_run(beng, 1)
    assert not st.any() and not st1.any()
    ref_trace, ref_state = np.concatenate([t2, t1]), fam.state(beng)
    ref_theta, _, ref_sc = beng._vi_resident(fam.K)

    assert not _start(beng, fam, rows, tables, prior).any()
    identity = [np.arange(c) for c in counts]
    trace, n_done, status = fam.svi_run(beng, 3, 1.0, np.ones(B), np.array(counts), rows=[identity] * 2, resident_start=True)
    assert not status.any() and list(n_done) == [3] * B
    assert np.array_equal(trace, ref_trace)
    assert tg._states_equal(fam.state(beng), ref_state) is None
    theta, S, sc = beng._vi_resident(fam.K)
    assert np.array_equal(theta, ref_theta) and np.array_equal(sc[:, 0], ref_sc[:, 0])
    for a, b in zip(S, S2):
        assert np.array_equal(a.n, b.n) and np.array_equal(a.sx, b.sx) and np.array_equal(a.sxx, b.sxx)


# ---- 2. the blend carries the host's bits; the init mode -----------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES + [DEEP], ids=ids(FAMILIES + [DEEP]))
def test_blend_and_init_carry_the_host_bits(beng, fam):
    counts = COUNTS if fam is not DEEP else (40, 64)
    B = len(counts)
    rows, tables, prior = fam.problems(counts, seed=23)
    start = _posterior_state(beng, fam, rows, tables, prior)
    _, other, _ = fam.problems(counts, seed=24)                     # the step's statistics: those of other tables
    for rho in (0.5, 0.3, 1e-3):
        assert not _start(beng, fam, rows, other, prior, start).any()
        # the init mode: exactly the uploaded natural parameters, and the image of its own canonical form
        init = fam.state(beng)
        for name in fam.NAT:
            assert np.array_equal(init[name], start[name]), name
        theta, S, _ = beng._vi_resident(fam.K)
        for b in range(B):
            assert np.array_equal(theta[b], fam.image(init, b)), b
        scale = 7. / 40.
        trace, n_done, status = fam.svi_run(beng, 1, rho, np.full(B, scale), np.zeros(B, dtype=np.int64), rows=[],
                                            resident_start=True)
        assert not status.any() and list(n_done) == [1] * B and np.all(np.isfinite(trace))
        new = fam.state(beng)
        for b in range(B):
            want = fam.host_blend(fam.prior_of(prior, b), {k: start[k][b] for k in fam.NAT}, S[b], rho, scale)
            for name in fam.NAT:
                assert np.array_equal(new[name][b], want[name]), (rho, b, name)
        theta, _, _ = beng._vi_resident(fam.K)
        for b in range(B):
            assert np.array_equal(theta[b], fam.image(new, b)), b


# ---- 3. the driver against the host route --------------------------------------------------------------------------------------
@pytest.mark.parametrize("randomize", [False, True])
@pytest.mark.parametrize("name,step,tol,ptol", HOST_CASES)
def test_resident_driver_equals_the_host_route(engine, beng, monkeypatch, name, step, tol, ptol, randomize):
    """Measured on the MI355X (12 iterations, batch 64; largest relative difference to the host route over the 4 models):
    see DESIGN.md section 4i."""
    kw = dict(randomize=randomize, maxiter=12, step_size=step, batch_size=64, sample_likelihood=False, numpy_seeds=NUMPY_SEEDS,
              python_seeds=PYTHON_SEEDS, engine=beng)
    models, data = _models(name, engine)
    if name.startswith("ilr"):
        assert _ilr_resident_reason(models[0])[0] is None
    with monkeypatch.context() as mp:
        for what in ("upload", "estep", "weighted_stats"):
            mp.setattr(HipEngine, what, _refuse)
        vlbs = meanfield_stochastic_descent_batched(models, data, resident=True, chunk=5, **kw)
    assert [len(v) for v in vlbs] == [12] * len(models)
    assert vlbs[0] == vlbs[1]
    hosts, _ = _models(name, engine)
    ref = meanfield_stochastic_descent_batched(hosts, data, resident=False, **kw)
    worst = [0., 0.]
    for m, h, v, r in zip(models, hosts, vlbs, ref):
        worst[0] = max(worst[0], rel_err(np.array(v), np.array(r)))
        worst[1] = max([worst[1]] + [rel_err(a, b) for a, b in zip(_posterior(m), _posterior(h))])
    print(f"{name} randomize={randomize}: largest difference to the host route: trace {worst[0]:.2e}, posterior {worst[1]:.2e}")
    assert worst[0] < tol and worst[1] < ptol


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def _svi(eng, fam, rows, tables, prior, state, chunks, sizes, draws=None, seeds=None, rho=0.4):
    """start from `state`, svi_run per chunk on the index lists `draws` (or Philox seeds) -> (trace, status, final state)."""
    assert not _start(eng, fam, rows, tables, prior, state).any()
    counts = np.array([len(r) for r in rows], dtype=float)
    scale = np.minimum(np.asarray(sizes) / np.maximum(counts, 1.), 1.)
    out, at = [], 0
    for n in chunks:
        out.append(fam.svi_run(eng, n, rho, scale, np.asarray(sizes), rows=None if draws is None else draws[at:at + n], seeds=seeds))
        at += n
    return np.concatenate([t for t, _, _ in out]), out[-1][2], fam.state(eng)


@pytest.mark.parametrize("fam", FAMILIES, ids=ids(FAMILIES))
def test_a_problem_does_not_depend_on_its_batch(beng, fam):
    rows, tables, prior = fam.problems(COUNTS, seed=31)
    start = _posterior_state(beng, fam, rows, tables, prior)
    sizes = (16, 33, 64)
    draws = _draws(COUNTS, sizes, 3, seed=5)
    trace, status, state = _svi(beng, fam, rows, tables, prior, start, [3], sizes, draws)
    assert not status.any() and np.all(np.isfinite(trace))
    for i in range(3):
        one = {k: v[i:i + 1] for k, v in start.items()}
        t1, s1, st1 = _svi(beng, fam, rows[i:i + 1], tables[i:i + 1], fam.one(prior, i), one, [3], sizes[i:i + 1],
                           [d[i:i + 1] for d in draws])
        assert np.array_equal(t1[:, 0], trace[:, i]), i
        assert tg._states_equal(state, st1, (i, 0)) is None, i


@pytest.mark.parametrize("fam", [FAMILIES[1], FAMILIES[4]], ids=ids([FAMILIES[1], FAMILIES[4]]))
def test_shared_batch_equals_the_batch_of_copies(beng, fam):
    B = 3
    rows, tables, prior = fam.problems((150,) * B, seed=41)
    Z = rows[0]
    start = _posterior_state(beng, fam, [Z] * B, tables, prior)
    sizes, draws = (32,) * B, _draws((150,) * B, (32,) * B, 4, seed=6)
    t_copies, _, s_copies = _svi(beng, fam, [Z] * B, tables, prior, start, [4], sizes, draws)
    beng.upload_shared(Z, B)
    beng.weighted_stats(tables)
    fam.set_prior(beng, prior)
    assert not fam.set_state(beng, start).any()
    t_shared, _, st = fam.svi_run(beng, 4, 0.4, np.full(B, 32 / 150.), np.array(sizes), rows=draws)
    assert not st.any() and np.array_equal(t_shared, t_copies)
    assert tg._states_equal(fam.state(beng), s_copies) is None


@pytest.mark.parametrize("fam", [FAMILIES[0], FAMILIES[4]], ids=ids([FAMILIES[0], FAMILIES[4]]))
@pytest.mark.parametrize("philox", [False, True])
def test_chunked_runs_equal_one_run(beng, fam, philox):
    """svi_run(6) = svi_run(2) then svi_run(4): on the same index lists, and with Philox seeds (the iteration counter of the
    draws runs on across calls)."""
    rows, tables, prior = fam.problems(COUNTS, seed=51)
    start = _posterior_state(beng, fam, rows, tables, prior)
    sizes = (16, 64, 48)
    kw = dict(seeds=[3, 4, 5]) if philox else dict(draws=_draws(COUNTS, sizes, 6, seed=7))
    t6, _, s6 = _svi(beng, fam, rows, tables, prior, start, [6], sizes, **kw)
    t24, _, s24 = _svi(beng, fam, rows, tables, prior, start, [2, 4], sizes, **kw)
    assert np.all(np.isfinite(t6)) and np.array_equal(t6, t24)
    assert tg._states_equal(s6, s24) is None


# ---- 5. the device's indices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [FAMILIES[0], FAMILIES[3]], ids=ids([FAMILIES[0], FAMILIES[3]]))
def test_device_indices_are_the_host_mirror(beng, fam):
    """index_rng='philox' = explicit host indices min(int(u N_b), N_b - 1), u = mimo_philox_uniform(seed_b, slot, t): with a problem
    of one row and problems smaller than their minibatch (draws with replacement)."""
    counts, sizes, seeds = (40, 1, 10), (16, 16, 16), [11, 12, 2 ** 63 + 5]
    rows, tables, prior = fam.problems(counts, seed=61)
    start = _posterior_state(beng, fam, rows, tables, prior)
    draws = []
    for t in range(5):
        draws.append([np.minimum((philox_uniforms(seeds[b], np.arange(sizes[b]), t) * float(counts[b])).astype(np.int64),
                                 counts[b] - 1) for b in range(3)])
        assert all(np.array_equal(d, philox_indices(seeds[b], counts[b], sizes[b], t)) for b, d in enumerate(draws[-1]))
    assert len(np.unique(draws[0][0])) > 8 and not draws[0][1].any()
    t_dev, st, s_dev = _svi(beng, fam, rows, tables, prior, start, [2, 3], sizes, seeds=seeds)
    t_host, _, s_host = _svi(beng, fam, rows, tables, prior, start, [5], sizes, draws=draws)
    assert not st.any() and np.all(np.isfinite(t_dev)) and np.array_equal(t_dev, t_host)
    assert tg._states_equal(s_dev, s_host) is None


# ---- 6. failures ---------------------------------------------------------------------------------------------------------------------
def _bad_prior(fam, prior, how):
    """Problem 1's prior such that the blend leaves an indefinite block (bit 1) or a digamma argument <= 0 (bit 2)."""
    if isinstance(fam, Gmm):
        bad = {k: v.copy() for k, v in prior.items()}
        if how == 1:
            bad["pc"][1, 2] = -1e4 * np.eye(fam.D)
        else:
            bad["pd"][1] = -1e6
    else:
        bad = ti._copy(prior)
        if how == 1:
            bad["experts"][2][1, 2] = -1e4 * np.eye(fam.dy)
        else:
            bad["experts"][3][1] = -1e6
    return bad


@pytest.mark.parametrize("how", [1, 2])
@pytest.mark.parametrize("fam", [Gmm(2, 4), Ilr(2, 2, 4, 'dirichlet')], ids=["gmm", "ilr"])
def test_a_failing_problem_stops_alone_and_keeps_its_block(beng, fam, how):
    rows, tables, prior = fam.problems(COUNTS, seed=71)
    start = _posterior_state(beng, fam, rows, tables, prior)
    bad = _bad_prior(fam, prior, how)
    sizes, draws = (16, 32, 64), _draws(COUNTS, (16, 32, 64), 3, seed=8)
    assert not _start(beng, fam, rows, tables, bad, start).any()           # the starting posterior itself is sound
    before = fam.state(beng)
    scale = np.array(sizes) / np.array(COUNTS, dtype=float)
    trace, n_done, status = fam.svi_run(beng, 3, 0.5, scale, np.array(sizes), rows=draws)
    assert list(status) == [0, how, 0] and list(n_done) == [3, 0, 3]
    assert np.all(np.isnan(trace[:, 1])) and np.all(np.isfinite(trace[:, [0, 2]]))
    state = fam.state(beng)
    assert tg._states_equal(state, before, (1, 1)) is None               # the failed problem keeps its last complete block
    for i in (0, 2):                                                       # the others: the numbers they have alone
        one = {k: v[i:i + 1] for k, v in start.items()}
        t1, _, s1 = _svi(beng, fam, rows[i:i + 1], tables[i:i + 1], fam.one(prior, i), one, [3], sizes[i:i + 1],
                         [d[i:i + 1] for d in draws], rho=0.5)
        assert np.array_equal(t1[:, 0], trace[:, i]) and tg._states_equal(state, s1, (i, 0)) is None


def test_the_driver_names_the_failing_problem(engine, beng):
    build, data = tg._gmm_batch(engine, counts=(120, 64, 200))
    kw = dict(randomize=False, maxiter=3, step_size=0.5, batch_size=32, sample_likelihood=False, numpy_seeds=[1, 2, 3],
              python_seeds=[4, 5, 6], engine=beng, resident=True)
    models = build()
    blk = native_sweep._prior_block(models[1].components.prior)
    pc = blk[2].copy()
    pc[0] = -1e6 * np.eye(2)
    models[1].components.prior._memo['sweep_c64'] = (blk[0], blk[1], pc, blk[3], blk[4])
    with pytest.raises(np.linalg.LinAlgError, match="problem 1"):
        meanfield_stochastic_descent_batched(models, data, **kw)
    models = build()
    blk = native_sweep._prior_block(models[2].components.prior)
    models[2].components.prior._memo['sweep_c64'] = (blk[0], blk[1], blk[2], np.full_like(blk[3], -1e6), blk[4])
    with pytest.raises(FloatingPointError, match="problem 2"):
        meanfield_stochastic_descent_batched(models, data, index_rng='philox', seeds=[7, 8, 9], **kw)


def _raw_run(eng, fam, iters, rho, scale, rows, sizes, seeds=None, flags=0):
    B = eng.B
    sel_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scale = np.ascontiguousarray(scale, dtype=float)
    trace, n_done, status = np.full((iters, B), -7.), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    call = eng._lib.mimo_svi_run_batched if isinstance(fam, Gmm) else eng._lib.mimo_svi_ilr_run_batched
    rc = call(eng._ctx, fam.K, iters, rho, scale.ctypes.data, None if rows is None else rows.ctypes.data, sel_off.ctypes.data,
              None if seeds is None else seeds.ctypes.data, flags, trace.ctypes.data, n_done.ctypes.data, status.ctypes.data)
    return rc, eng._lib.mimo_last_error(eng._ctx).decode(), trace


@pytest.mark.parametrize("fam", [FAMILIES[0], FAMILIES[3]], ids=ids([FAMILIES[0], FAMILIES[3]]))
def test_a_bad_index_in_a_later_iteration_is_refused_before_anything_runs(beng, fam):
    rows, tables, prior = fam.problems(COUNTS, seed=81)
    start = _posterior_state(beng, fam, rows, tables, prior)
    assert not _start(beng, fam, rows, tables, prior, start).any()
    before, theta0 = fam.state(beng), beng._vi_resident(fam.K)[0]
    sizes = (16, 16, 16)
    idx = np.ascontiguousarray(np.concatenate([np.concatenate(d) for d in _draws(COUNTS, sizes, 4, seed=9)]).reshape(4, 48))
    idx[2, 16 + 3] = 64                                                     # iteration 2, problem 1 (N = 64), entry 3
    rc, msg, trace = _raw_run(beng, fam, 4, 0.5, np.full(3, 0.25), idx, sizes)
    assert rc == _lib.E_INVALID and "iteration 2" in msg and "problem 1" in msg and "index 64" in msg
    assert np.all(trace == -7.)
    assert tg._states_equal(fam.state(beng), before) is None and np.array_equal(beng._vi_resident(fam.K)[0], theta0)
    idx[2, 16 + 3] = 63
    rc, msg, trace = _raw_run(beng, fam, 4, 0.5, np.full(3, 0.25), idx, sizes)
    assert rc == 0 and np.all(np.isfinite(trace))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    gm, il = Gmm(2, 4), Ilr(1, 1, 4, 'stick-breaking')
    rows, tables, prior = gm.problems(COUNTS, seed=91)
    _, _, iprior = il.problems(COUNTS, seed=91)
    eng = BatchedHipEngine(0)
    sizes, sc = (16, 16, 16), np.full(3, 0.25)
    idx = np.ascontiguousarray(np.concatenate([np.concatenate(d) for d in _draws(COUNTS, sizes, 2, seed=1)]).reshape(2, 48))
    eng.upload(rows)
    eng.weighted_stats(tables)
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, idx, sizes)                  # no prior block
    assert rc == _lib.E_STATE and "prior" in msg
    status = np.zeros(3, dtype=np.int32)
    st = gm.prior_as_state(prior)
    rc = eng._lib.mimo_svi_state_batched(eng._ctx, 4, *(np.ascontiguousarray(st[n]).ctypes.data for n in gm.NAT), status.ctypes.data)
    assert rc == _lib.E_STATE and "prior" in eng._lib.mimo_last_error(eng._ctx).decode()
    gm.set_prior(eng, prior)
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, idx, sizes)                  # a prior block, no state
    assert rc == _lib.E_STATE and "mimo_svi_state_batched" in msg
    assert not gm.set_state(eng, st).any()
    rc, msg, _ = _raw_run(eng, il, 2, 0.5, sc, idx, sizes)                  # the other family's prior block
    assert rc == _lib.E_STATE and "that of mixtures of Gaussians" in msg
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, idx, sizes, flags=_lib.F_NO_STATS)
    assert rc == _lib.E_INVALID and "MIMO_F_SVI_RESIDENT_START" in msg    # a flag outside the defined set
    for bad_rho in (0., 1.5, float('nan')):
        rc, msg, _ = _raw_run(eng, gm, 2, bad_rho, sc, idx, sizes)
        assert rc == _lib.E_INVALID and "step_size" in msg
    for bad in (0., -1., float('inf'), float('nan')):
        rc, msg, _ = _raw_run(eng, gm, 2, 0.5, np.array([0.25, bad, 0.25]), idx, sizes)
        assert rc == _lib.E_INVALID and "scale[1]" in msg
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, None, sizes)
    assert rc == _lib.E_INVALID and "seeds" in msg                          # neither indices nor seeds
    eng.estep(np.zeros((3, 4)), np.zeros((3, 4, 2)), np.stack([np.stack([np.eye(2)] * 4)] * 3), stats=False)
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, idx[:1], sizes, flags=_lib.F_SVI_RESIDENT_START)
    assert rc == _lib.E_STATE and "statistics" in msg                       # the resident start without resident statistics
    rc, msg, trace = _raw_run(eng, gm, 2, 0.5, sc, idx, sizes)              # ... and the loop is still usable
    assert rc == 0 and np.all(np.isfinite(trace))
    eng.upload(rows)                                                        # an upload drops the priors and the state
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, idx, sizes)
    assert rc == _lib.E_STATE and "prior" in msg
    eng.weighted_stats(tables)
    gm.set_prior(eng, prior)                                                # a new prior block drops the state
    rc, msg, _ = _raw_run(eng, gm, 2, 0.5, sc, idx, sizes)
    assert rc == _lib.E_STATE and "mimo_svi_state_batched" in msg
    bad = {k: v.copy() for k, v in st.items()}
    bad["qc"][2, 1, 0, 0] = np.nan
    rc = eng._lib.mimo_svi_state_batched(eng._ctx, 4, *(np.ascontiguousarray(bad[n]).ctypes.data for n in gm.NAT), status.ctypes.data)
    assert rc == _lib.E_INVALID and "qc of problem 2" in eng._lib.mimo_last_error(eng._ctx).decode()
    eng.close()
