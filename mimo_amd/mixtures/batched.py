"""Mean-field coordinate descent and Gibbs sampling of B independent mixtures with ONE batched pass per iteration / sweep
(mimo_amd.batched.BatchedHipEngine): what the reference does with joblib.Parallel over B fits
(examples/ilr/evaluate_sinc_parallel.py) or with random restarts of one model.

VI: per iteration each model runs the host step of its own meanfield_iteration, in model order (conjugate update — the
native sweep where it applies —, canonical form), then one batched pass over all B data sets, then, per model, the
likelihood draws, the prior terms of the bound and the bound itself.  A model stops at the iteration where its solo
run would stop; after that it is neither updated nor appended to (its last parameters stay in the batch).

Gibbs: per sweep each model runs the host half of its solo resample sweep, in model order (parameter and gating draws,
canonical form, host uniforms), then one batched label pass draws every model's labels and their statistics.

SVI: per outer iteration each model draws its minibatch indices, in model order; one batched pass over the chosen rows
of every model's resident data (BatchedHipEngine.estep(rows=...): the rows are gathered on the device, nothing but the
indices is uploaded) gives the minibatch statistics; each model takes its natural-gradient step (_svi_step, the step of
its solo meanfield_stochastic_descent); one batched pass over all rows gives the bounds.  resident=True: the step runs on the
device as well (BatchedHipEngine.svi_run), `chunk` iterations per call, and the posteriors come back once.

Nested VI (meanfield_coordinate_descent_nested): the M inner mixtures of a mixture of mixtures (mixtures/hgmm.py) are the
problems of ONE shared batch over one copy of the data; their inner descents run in lockstep on weighted batched passes, and
the outer responsibilities — the weights of those passes — are computed and kept on the device."""
import copy
import random
from contextlib import contextmanager, nullcontext

import numpy as np
import numpy.random as npr

from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import SuffStats
from mimo_amd.distributions import native_sweep as _native_sweep
from mimo_amd.distributions.lingauss import joint_rows
from mimo_amd.mixtures.gmm import BayesianMixtureOfGaussians, _component_stats
from mimo_amd.mixtures.ilr import BayesianMixtureOfLinearGaussians
from mimo_amd.utils.data import sample_indices


def _rows(model, d):
    """The model's data rows as its solo driver uploads them (ILR: scaled per model, z = [x, y])."""
    if isinstance(model, BayesianMixtureOfGaussians):
        if model._structure() != 'full':
            raise ValueError("the batched pass covers symmetric precision blocks only (full structure)")
        return np.ascontiguousarray(np.asarray(d, dtype=float).reshape(-1, model.dim))
    x, y = d
    return np.ascontiguousarray(joint_rows(*model._scaled(x, y)))


def _begin(model, S):
    """Host step of meanfield_iteration before its pass: -> (canonical form, prior-terms callable)."""
    if isinstance(model, BayesianMixtureOfGaussians):
        fused = _native_sweep.gmm_vi_sweep(model.gating, model.components, _component_stats(S, model.components),
                                           S.gating_counts)
        if fused is not None:
            return fused
    model._update_from_stats(S, sample=False)
    return model.canonical_expected(), model._vlb_prior_terms


def _stack(canons):
    return tuple(np.stack([np.asarray(cn[i], dtype=float) for cn in canons]) for i in range(3))


def _check_models(models, data):
    """One class, one size and one set of dimensions for all: -> (models, data, class)."""
    models, data = list(models), list(data)
    B = len(models)
    if B == 0 or len(data) != B:
        raise ValueError(f"{B} models and {len(data)} data sets")
    cls = type(models[0])
    if cls not in (BayesianMixtureOfGaussians, BayesianMixtureOfLinearGaussians) or any(type(m) is not cls for m in models):
        raise ValueError("the models must all be BayesianMixtureOfGaussians or all BayesianMixtureOfLinearGaussians")
    dims = [(m.size, m.dim) if cls is BayesianMixtureOfGaussians else (m.size, m.input_dim, m.output_dim, m.affine)
            for m in models]
    if any(d != dims[0] for d in dims):
        raise ValueError(f"the models differ in size or dimensions: {dims}")
    return models, data, cls


def _per_model(values, B, default, what):
    values = [default] * B if values is None else list(values)
    if len(values) != B:
        raise ValueError(f"{len(values)} {what} for {B} models")
    return values


def _random_start(engine, K, init_rng, seeds):
    """random_start (mixtures/gmm.py) of every model in one batched pass over the data the engine holds.
    init_rng='host'  : numpy.random.rand(K, N_b) per model, in model order — what B solo runs draw one after another;
    init_rng='philox': drawn on the device, model i from the Philox stream keyed by seeds[i] (counter (row, k))."""
    if init_rng == 'philox':
        return engine.random_resp_stats(K, seeds)
    if init_rng != 'host':
        raise ValueError(init_rng)
    tables = []
    for n in np.diff(engine.row_off):
        resp = npr.rand(K, int(n))
        resp /= np.sum(resp, axis=0)
        tables.append(resp)
    return engine.weighted_stats(tables)


def _resident_reason(model, sample_likelihood):
    """Why the device-resident loop does not take this model (None: it does) — the family gmm_vi_sweep covers with untied
    blocks: a mixture of Gaussians, Dirichlet gating, full Normal-Wishart components."""
    from mimo_amd.distributions.bayesian import CategoricalWithDirichlet, StackedGaussiansWithNormalWisharts
    from mimo_amd.distributions.composite import StackedNormalWisharts
    from mimo_amd.distributions.gating import Dirichlet
    if sample_likelihood:
        return "sample_likelihood=True (the loop makes no per-iteration likelihood draws)"
    if type(model) is not BayesianMixtureOfGaussians:
        return f"{type(model).__name__} is not a BayesianMixtureOfGaussians"
    gating, comps = model.gating, model.components
    if type(gating) is not CategoricalWithDirichlet or type(gating.prior) is not Dirichlet\
            or type(gating.posterior) is not Dirichlet:
        return "the gating is not a CategoricalWithDirichlet with Dirichlet prior and posterior"
    if type(comps) is not StackedGaussiansWithNormalWisharts:
        return f"the components are {type(comps).__name__} (tied or other blocks), not StackedGaussiansWithNormalWisharts"
    if type(comps.prior) is not StackedNormalWisharts or type(comps.posterior) is not StackedNormalWisharts:
        return "the components' prior and posterior are not StackedNormalWisharts"
    if model._structure() != 'full':
        return f"the structure is {model._structure()!r}, not 'full'"
    return None


def _resident_descent(models, engine, maxiter, tol, chunk):
    """The loop of meanfield_coordinate_descent_batched(resident=True) behind the start: the statistics of the start lie on the
    device; priors up once, vi_run in chunks, state back once."""
    B, K = len(models), models[0].size
    maxiter, chunk = int(maxiter), int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk} < 1")
    vlbs = [[] for _ in range(B)]
    if maxiter <= 0:
        return vlbs
    blocks = [_native_sweep._prior_block(m.components.prior) for m in models]
    engine.vi_set_prior(np.stack([np.asarray(m.gating.prior.alphas, dtype=float) for m in models]),
                        *(np.stack([blk[j] for blk in blocks]) for j in range(5)))
    left, stopped = maxiter, np.zeros(B, dtype=bool)
    while left > 0 and not stopped.all():
        n = min(chunk, left)
        trace, n_done, status = engine.vi_run(K, n, tol)
        left -= n
        for i in np.flatnonzero(status):
            if status[i] & 1:
                raise np.linalg.LinAlgError(f"problem {int(i)}: Matrix is not positive definite (a component's block "
                                            "c - kappa m m' of its posterior)")
            raise FloatingPointError(f"problem {int(i)}: the canonical form or the bound of its posterior is not finite")
        for i in range(B):
            vlbs[i].extend(float(v) for v in trace[:int(n_done[i]), i])
            # (the device's own rule, on the same doubles: a problem that stopped at a chunk's last iteration is seen here)
            stopped[i] = n_done[i] < n or (len(vlbs[i]) > 1 and abs(vlbs[i][-1] - vlbs[i][-2]) < tol)
    _write_gmm_state(models, engine.vi_state(K), vlbs)
    return vlbs


def _write_gmm_state(models, state, vlbs, stream=None):
    """The posterior blocks of a resident GMM loop (BatchedHipEngine.vi_state) into the models that appended a bound, as the
    host-native sweep writes them, with memos; then one _refresh_likelihoods() per model (inside stream(i), if given)."""
    from mimo_amd.utils.abstraction import Statistics as Stats
    part = lambda name, i: np.ascontiguousarray(state[name][i])
    for i, m in enumerate(models):
        if not vlbs[i]:
            continue
        post = m.components.posterior
        qb, nus, bb, W = part('qb', i), part('nus', i), part('bb', i), part('W', i)
        m.gating.posterior.alphas = part('alpha', i)
        post.params = (part('mus', i), qb, part('psis', i), nus)
        post._set_memo(nat=Stats([part('qa', i), qb, part('qc', i), part('qd', i)]), hld=part('hld', i),
                       estats=(bb, part('E2', i), - 0.5 * W, part('E4', i)), canon=(part('cc', i), bb, W), native=True)
        with stream(i) if stream is not None else nullcontext():
            m._refresh_likelihoods()


def meanfield_coordinate_descent_batched(models, data, randomize=True, maxiter=250, tol=1e-8, init_rng='host', seeds=None,
                                         sample_likelihood=True, engine=None, resident=False, chunk=8):
    """models: B BayesianMixtureOfGaussians with data a list of B `obs`, or B BayesianMixtureOfLinearGaussians with data a
    list of B `(x, y)`; one class, one size and one set of dimensions for all.  randomize / init_rng / seeds[i] /
    sample_likelihood as in the solo drivers (the random start is one batched table pass: the host draws are made in
    model order).  engine: a
    BatchedHipEngine (default: a new one on the device of the first model's engine).  Returns the B ELBO traces.

    resident=True: everything between two passes runs on the device (BatchedHipEngine.vi_run): the conjugate update, the
    canonical form, the prior terms of the bound and the stopping rule, `chunk` iterations per call; the posteriors come
    back once, at the end, and are written into the models as the host-native sweep writes them (then one
    _refresh_likelihoods() per model).  Only mixtures of Gaussians with a Dirichlet gating and untied Normal-Wishart
    components, and only sample_likelihood=False; anything else raises ValueError naming the reason.  A problem one of whose
    blocks is not positive definite raises numpy.linalg.LinAlgError naming the problem, as the NumPy route does; one whose
    canonical form or bound is not finite raises FloatingPointError naming the problem."""
    models, data, cls = _check_models(models, data)
    B = len(models)
    seeds = _per_model(seeds, B, 0, "seeds")
    if resident:
        for i, m in enumerate(models):
            why = _resident_reason(m, sample_likelihood)
            if why is not None:
                raise ValueError(f"resident=True does not cover model {i}: {why}")
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    engine.upload([_rows(m, d) for m, d in zip(models, data)])

    if randomize:
        S = _random_start(engine, models[0].size, init_rng, seeds)
    else:
        canons = [m.canonical_expected() for m in models]
        S, _ = engine.estep(*_stack(canons))
    if resident:
        return _resident_descent(models, engine, maxiter, tol, chunk)
    canons = [None] * B
    vlbs = [[] for _ in range(B)]
    active = list(range(B))
    for _ in range(maxiter):
        if not active:
            break
        prior = {}
        for i in active:
            canons[i], prior[i] = _begin(models[i], S[i])
        Sb, sc = engine.estep(*_stack(canons))
        still = []
        for i in active:
            if sample_likelihood:
                models[i]._refresh_likelihoods()
            vlbs[i].append(prior[i]() + sc[i, 0])
            S[i] = Sb[i]
            if not (len(vlbs[i]) > 1 and abs(vlbs[i][-1] - vlbs[i][-2]) < tol):
                still.append(i)
        active = still
    return vlbs


def _ilr_resident_reason(model):
    """Why the device-resident ILR loop does not take this model (None: it does) -> (reason, gating kind): affine, untied
    matrix-normal-Wishart experts, an untied Normal-Wishart basis, a Dirichlet or a stick-breaking gating, within the batched
    pass's own limits."""
    from mimo_amd.distributions.bayesian import (CategoricalWithDirichlet, CategoricalWithStickBreaking,
                                                 StackedGaussiansWithNormalWisharts,
                                                 StackedLinearGaussiansWithMatrixNormalWisharts)
    from mimo_amd.distributions.composite import StackedMatrixNormalWisharts, StackedNormalWisharts
    from mimo_amd.distributions.gating import Dirichlet, TruncatedStickBreaking
    if type(model) is not BayesianMixtureOfLinearGaussians:
        return f"{type(model).__name__} is not a BayesianMixtureOfLinearGaussians", None
    gating, basis, experts = model.gating, model.basis, model.models
    kind = None
    if type(gating) is CategoricalWithDirichlet and type(gating.prior) is Dirichlet and type(gating.posterior) is Dirichlet:
        kind = 'dirichlet'
    elif type(gating) is CategoricalWithStickBreaking and type(gating.prior) is TruncatedStickBreaking\
            and type(gating.posterior) is TruncatedStickBreaking:
        kind = 'stick-breaking'
    if kind is None:
        return "the gating is neither a CategoricalWithDirichlet (Dirichlet) nor a CategoricalWithStickBreaking "\
               "(TruncatedStickBreaking)", None
    if type(basis) is not StackedGaussiansWithNormalWisharts or type(basis.prior) is not StackedNormalWisharts\
            or type(basis.posterior) is not StackedNormalWisharts:
        return f"the basis is {type(basis).__name__} with {type(basis.prior).__name__} (tied or other blocks), not "\
               "StackedGaussiansWithNormalWisharts with StackedNormalWisharts", kind
    if type(experts) is not StackedLinearGaussiansWithMatrixNormalWisharts\
            or type(experts.prior) is not StackedMatrixNormalWisharts or type(experts.posterior) is not StackedMatrixNormalWisharts:
        return f"the experts are {type(experts).__name__} with {type(experts.prior).__name__} (tied or other blocks), not "\
               "StackedLinearGaussiansWithMatrixNormalWisharts with StackedMatrixNormalWisharts", kind
    if not model.affine or experts.prior.column_dim != model.input_dim + 1:
        return "the experts are not affine (column_dim = input_dim + 1)", kind
    dx, dy, K = model.input_dim, model.output_dim, model.size
    if dx < 1 or dy < 1 or dx + dy > 16 or not 1 <= K <= 128:
        return f"input_dim = {dx}, output_dim = {dy}, size = {K} are outside dx, dy >= 1, dx + dy <= 16, K <= 128", kind
    return None, kind


def meanfield_coordinate_descent_batched_ilr(models, data, randomize=True, maxiter=250, tol=1e-8, init_rng='host', seeds=None,
                                             engine=None, chunk=8):
    """Mean-field coordinate descent of B BayesianMixtureOfLinearGaussians with everything between two passes on the device
    (BatchedHipEngine.vi_ilr_run): the update of the basis, of the experts and of the gating from the resident joint
    statistics, the joint canonical form, the prior terms of the bound and the stopping rule, `chunk` iterations per call.
    What meanfield_coordinate_descent_batched(models, data, sample_likelihood=False) computes with a host step per model and
    iteration; models / data / randomize / init_rng / seeds / engine as there.  The start is the same (upload, then the random
    start or one plain pass); then the priors go up once, the loop runs in chunks, and the posteriors come back once and are
    written into the models as the host route leaves them (gating, basis, experts with their memos; then one
    _refresh_likelihoods() per model).  Returns the B ELBO traces.

    Covered: affine, untied experts (StackedLinearGaussiansWithMatrixNormalWisharts over StackedMatrixNormalWisharts with
    column_dim = input_dim + 1), an untied Normal-Wishart basis, and one gating kind for the whole batch, Dirichlet or
    stick-breaking; input_dim + output_dim <= 16, size <= 128.  Anything else raises ValueError naming the model and the
    reason before anything is uploaded or drawn.  A problem one of whose blocks is not positive definite raises
    numpy.linalg.LinAlgError naming the problem; one whose canonical form or bound is not finite raises FloatingPointError."""
    models, data = list(models), list(data)
    B = len(models)
    if B == 0 or len(data) != B:
        raise ValueError(f"{B} models and {len(data)} data sets")
    kinds = []
    for i, m in enumerate(models):
        why, kind = _ilr_resident_reason(m)
        if why is not None:
            raise ValueError(f"the resident ILR loop does not cover model {i}: {why}")
        kinds.append(kind)
    if any(k != kinds[0] for k in kinds):
        raise ValueError(f"the resident ILR loop takes one gating kind per batch, got {kinds}")
    models, data, _ = _check_models(models, data)
    seeds = _per_model(seeds, B, 0, "seeds")
    maxiter, chunk = int(maxiter), int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk} < 1")
    if init_rng not in ('host', 'philox'):
        raise ValueError(init_rng)
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    engine.upload([_rows(m, d) for m, d in zip(models, data)])
    K, stick = models[0].size, kinds[0] == 'stick-breaking'
    if randomize:
        _random_start(engine, K, init_rng, seeds)
    else:
        engine.estep(*_stack([m.canonical_expected() for m in models]))
    vlbs = [[] for _ in range(B)]
    if maxiter <= 0:
        return vlbs

    arr = lambda v: np.asarray(v, dtype=float)
    bblocks = [_native_sweep._prior_block(m.basis.prior) for m in models]
    mblocks = [_native_sweep._prior_block(m.models.prior) for m in models]
    engine.vi_ilr_set_prior(kinds[0],
                            np.stack([arr(m.gating.prior.gammas if stick else m.gating.prior.alphas) for m in models]),
                            np.stack([arr(m.gating.prior.deltas) for m in models]) if stick else None,
                            tuple(np.stack([blk[j] for blk in bblocks]) for j in range(5)),
                            tuple(np.stack([blk[j] for blk in mblocks]) for j in range(5)))
    left, stopped = maxiter, np.zeros(B, dtype=bool)
    while left > 0 and not stopped.all():
        n = min(chunk, left)
        trace, n_done, status = engine.vi_ilr_run(K, n, tol)
        left -= n
        for i in np.flatnonzero(status):
            if status[i] & 1:
                raise np.linalg.LinAlgError(f"problem {int(i)}: Matrix is not positive definite (a block of a component's "
                                            "posterior: the basis' c - kappa m m', the experts' K or c - M K M')")
            raise FloatingPointError(f"problem {int(i)}: the canonical form or the bound of its posterior is not finite")
        for i in range(B):
            vlbs[i].extend(float(v) for v in trace[:int(n_done[i]), i])
            stopped[i] = n_done[i] < n or (len(vlbs[i]) > 1 and abs(vlbs[i][-1] - vlbs[i][-2]) < tol)
    _write_ilr_state(models, engine.vi_ilr_state(K), vlbs, stick)
    return vlbs


def _write_ilr_state(models, state, vlbs, stick, stream=None):
    """The posterior blocks of a resident ILR loop (BatchedHipEngine.vi_ilr_state) into the models that appended a bound, as
    the host route leaves them (gating, basis, experts with their memos); then one _refresh_likelihoods() per model (inside
    stream(i), if given)."""
    from mimo_amd.utils.abstraction import Statistics as Stats
    part = lambda name, i: np.ascontiguousarray(state[name][i])
    for i, m in enumerate(models):
        if not vlbs[i]:
            continue
        if stick:
            m.gating.posterior.gammas, m.gating.posterior.deltas = part('g0', i), part('g1', i)
        else:
            m.gating.posterior.alphas = part('g0', i)
        post = m.basis.posterior
        qb, bb, W = part('qb', i), part('bb', i), part('W', i)
        post.params = (part('mus', i), qb, part('psis', i), part('nus', i))
        post._set_memo(nat=Stats([part('qa', i), qb, part('qc', i), part('qd', i)]), hld=part('hld', i),
                       estats=(bb, part('E2', i), - 0.5 * W, part('E4', i)), canon=(part('cc', i), bb, W), native=True)
        post = m.models.posterior
        Kq, psis, nus = part('m_Kq', i), part('m_psis', i), part('m_nus', i)
        post.params = (part('m_Ms', i), Kq, psis, nus)
        post._set_memo(nat=Stats([part('m_a', i), Kq, part('m_c', i), part('m_d', i)]), hld=part('m_hld', i),
                       estats=(part('m_E1', i), part('m_E2', i), - 0.5 * nus[:, None, None] * psis, part('m_E4', i)),
                       canon_affine=(part('m_cc', i), part('m_bb', i), part('m_W', i)))
        with stream(i) if stream is not None else nullcontext():
            m._refresh_likelihoods()


def _nested_setup(model, obs, engine):
    """The shared batch of a mixture of mixtures: its M inner mixtures over ONE copy of obs -> (inner mixtures, engine)."""
    from mimo_amd.mixtures.hgmm import BayesianMixtureOfMixtureOfGaussians
    if type(model) is not BayesianMixtureOfMixtureOfGaussians:
        raise ValueError("the nested drivers take a BayesianMixtureOfMixtureOfGaussians")
    inner = list(model.components)
    if len(inner) != model.cluster_size or any(m.size != inner[0].size or m.dim != model.dim for m in inner):
        raise ValueError("the inner mixtures must share one size and the outer model's dimension")
    obs = np.ascontiguousarray(np.asarray(obs, dtype=float).reshape(-1, model.dim))
    if engine is None:
        engine = BatchedHipEngine(getattr(inner[0].engine, 'device', 0))
    engine.set_structure('full')
    engine.upload_shared(obs, len(inner))
    return inner, engine


def _tied(S):
    """A full-structure block as the tied ('linear') update reads it: only the pooled second moment exists."""
    return SuffStats(S.n, S.sx, None, sxx_total=S.sxx.sum(0))


def _nested_canons(inner):
    """The inner mixtures' canonical forms with K equal W_k (the batched pass is full-structure only)."""
    return _stack([tuple(np.array(p, dtype=float) for p in m.canonical_expected()) for m in inner])


def expected_responsibilities_nested(model, obs, engine=None):
    """expected_responsibilities of a BayesianMixtureOfMixtureOfGaussians (mixtures/hgmm.py) -> (M, N): one batched pass
    that keeps the M inner log-normalisers on the device, the outer softmax there (outer_responsibilities), one copy out."""
    inner, engine = _nested_setup(model, obs, engine)
    engine.estep(*_nested_canons(inner), stats=False, keep_lse=True)
    engine.outer_responsibilities(model.gating.expected_log_gating())
    return np.stack(engine.get_row_weights())


def meanfield_coordinate_descent_nested(model, obs, randomize=True, maxiter=250, maxsubiter=5, maxsubsubiter=5, engine=None):
    """meanfield_coordinate_descent of a BayesianMixtureOfMixtureOfGaussians (mixtures/hgmm.py) with ONE shared batch of
    cluster_size problems: the M inner mixtures read one copy of obs, their inner descents run in lockstep — one weighted
    batched pass per inner iteration —, and the outer responsibilities are computed and kept on the device
    (BatchedHipEngine.outer_responsibilities): after the start no (M, N) table crosses PCIe.

    Per outer iteration: the gating update from the outer counts; the M inner descents (per inner iteration every
    still-active inner mixture runs its conjugate update, then one weighted pass with the resident weights gives each its
    next statistics and its bound; an inner mixture stops where its solo run stops — two bounds closer than the inner
    driver's default tol = 1e-8 — and is left alone from then on); one pass that keeps the inner log-normalisers; the outer
    step.  randomize: the outer start is numpy.random.rand(M, N), normalised, and at the first outer iteration each inner
    mixture starts from numpy.random.rand(K, N), normalised, times its outer weights, for m = 0 .. M - 1 in that order.
    numpy's global stream is consumed exactly as the solo driver consumes it (same seeds: same tables, same drawn point
    estimates, same state afterwards); the price is that the FIRST outer iteration of a random start is not in lockstep
    (see below).  Returns [] (the reference records no bound)."""
    inner, engine = _nested_setup(model, obs, engine)
    M, K, N = len(inner), inner[0].size, int(engine.row_off[1])
    tol = 1e-8
    resp = None
    if randomize:
        resp = npr.rand(M, N)
        resp /= np.sum(resp, axis=0)
        counts = np.sum(resp, axis=1)
    else:
        engine.estep(*_nested_canons(inner), stats=False, keep_lse=True)
        counts, _ = engine.outer_responsibilities(model.gating.expected_log_gating())
    def stopped(vlb):
        return len(vlb) > 1 and abs(vlb[-1] - vlb[-2]) < tol

    for it in range(int(maxiter)):
        model.gating.meanfield_update(None, counts)
        if it == 0 and randomize:
            # The solo stream: table of mixture 0, its inner iterations' gating draws, table of mixture 1, ...  A Dirichlet
            # draw takes a number of generator words that depends on its parameters, so mixture m's table can only be drawn
            # once mixture m - 1 has finished: this one outer iteration runs the inner descents one after another (each
            # pass still covers the whole batch; the other problems' blocks are not read).
            weights = resp                       # the only upload of an (M, N) table: the random start's
            for m in range(M):
                r = npr.rand(K, N)
                r /= np.sum(r, axis=0)
                tables = [np.zeros((K, N))] * M
                tables[m] = r * resp[m]
                Sm = engine.weighted_stats(tables)[m]
                vlb = []
                for _ in range(int(maxsubiter)):
                    inner[m]._update_from_stats(_tied(Sm), maxsubsubiter)
                    Sb, sc = engine.estep(*_nested_canons(inner), row_weights=weights)
                    weights = 'resident'
                    Sm = Sb[m]
                    vlb.append(inner[m]._vlb_prior_terms() + sc[m, 0])
                    if stopped(vlb):
                        break
        else:
            # Lockstep.  The gating draws the solo updates end with (likelihood.params = posterior.rvs()) read nothing but the
            # posterior and feed nothing here: each is postponed and replayed below in the solo order — mixture by mixture,
            # iteration by iteration — so numpy's stream, and every drawn point estimate, is the solo run's.
            S, _ = engine.estep(*_nested_canons(inner), row_weights='resident')
            vlbs, gatings = [[] for _ in range(M)], [[] for _ in range(M)]
            active = list(range(M))
            for _ in range(int(maxsubiter)):
                if not active:
                    break
                for m in active:
                    mix = inner[m]
                    mix.components.meanfield_update(None, None, maxsubsubiter,
                                                    stats=_component_stats(_tied(S[m]), mix.components))
                    mix.gating.meanfield_update(None, S[m].n, sample=False)
                    gatings[m].append(copy.deepcopy(mix.gating.posterior))
                Sb, sc = engine.estep(*_nested_canons(inner), row_weights='resident')
                still = []
                for m in active:
                    vlbs[m].append(inner[m]._vlb_prior_terms() + sc[m, 0])
                    S[m] = Sb[m]
                    if not stopped(vlbs[m]):
                        still.append(m)
                active = still
            for m in range(M):
                for posterior in gatings[m]:       # (the last one is the mixture's final posterior)
                    inner[m].gating.posterior = posterior
                    inner[m].gating.refresh_likelihood()
        engine.estep(*_nested_canons(inner), stats=False, keep_lse=True)
        counts, _ = engine.outer_responsibilities(model.gating.expected_log_gating())
    return []


class _NumpyStreams:
    """Model i's host work on its own stream of numpy's global legacy generator: the stream starts as
    numpy.random.seed(numpy_seeds[i]) and is swapped in (set_state) and out (get_state) around each piece of model i's
    work — in-place draws on the global generator (distributions/wishart.py: legacy_draws) land in the state read back.
    Without numpy_seeds the global stream is used as it stands, in model order."""

    def __init__(self, numpy_seeds, B):
        self.states = None
        if numpy_seeds is not None:
            numpy_seeds = _per_model(numpy_seeds, B, 0, "numpy seeds")
            self.caller = npr.get_state()
            self.states = []
            for sd in numpy_seeds:
                npr.seed(sd)
                self.states.append(npr.get_state())
            npr.set_state(self.caller)

    @contextmanager
    def of(self, i):
        if self.states is None:
            yield
            return
        npr.set_state(self.states[i])
        try:
            yield
        finally:
            self.states[i] = npr.get_state()

    def restore(self):
        if self.states is not None:
            npr.set_state(self.caller)


def _resample_params(model, S, param_rng):
    """The parameter half of a solo resample sweep (gmm.py: components -> gating; ilr.py: basis -> models -> gating)."""
    if isinstance(model, BayesianMixtureOfGaussians):
        model.components.resample(None, stats=_component_stats(S, model.components), rng=param_rng)
    else:
        bstats, mstats = model._block_stats(S)
        model.basis.resample(None, stats=bstats, rng=param_rng)
        model.models.resample(None, None, stats=mstats, rng=param_rng)
    model.gating.resample(None, counts=S.gating_counts)


def resample_batched(models, data, init_labels='prior', maxiter=1, label_rng='host', seeds=None, param_rngs=None,
                     numpy_seeds=None, engine=None):
    """Gibbs sampling of B models with one batched label pass per sweep: per model what its solo
    resample(data, init_labels, maxiter, label_rng=label_rng, seed=seeds[i], param_rng=param_rngs[i]) does, labels_ set.
    models / data as in meanfield_coordinate_descent_batched.  numpy_seeds: model i's host work (initial labels, parameter
    and gating draws, host uniforms) runs on its own numpy stream started as numpy.random.seed(numpy_seeds[i]), so the
    batch reproduces B solo runs each preceded by numpy.random.seed(numpy_seeds[i]); the caller's global numpy state is
    restored at the end.  Without numpy_seeds the global stream is consumed in model order within each sweep (at B = 1:
    the solo run's order)."""
    models, data, cls = _check_models(models, data)
    B = len(models)
    if init_labels not in ('random', 'prior', 'posterior'):
        raise ValueError(init_labels)
    if label_rng not in ('host', 'philox'):
        raise ValueError(label_rng)
    if int(maxiter) < 0:
        raise ValueError(f"maxiter = {maxiter} < 0")
    seeds = _per_model(seeds, B, 0, "seeds")
    param_rngs = _per_model(param_rngs, B, None, "parameter generators")
    rows = [_rows(m, d) for m, d in zip(models, data)]       # (validates the structure before any draw)
    streams = _NumpyStreams(numpy_seeds, B)
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    try:
        engine.upload(rows)
        K = models[0].size

        def draw(sweep, stats, return_labels):
            canons, u = [], [] if label_rng == 'host' else None
            for i, m in enumerate(models):
                with streams.of(i):
                    canons.append(m.likelihood.canonical())
                    if u is not None:
                        u.append(npr.random(size=(1, len(rows[i]))))
            return engine.gibbs_labels(*_stack(canons), seeds=None if u is not None else seeds, sweep=sweep, u=u,
                                       stats=stats, return_labels=return_labels)

        if init_labels == 'posterior':
            labels, S = draw(0, True, True)
        else:
            labels = []
            for i, m in enumerate(models):
                with streams.of(i):
                    N = len(rows[i])
                    labels.append(npr.choice(m.size, size=(N)) if init_labels == 'random' else m.gating.likelihood.rvs(N))
            S = engine.label_stats(labels, K)
        for it in range(int(maxiter)):
            for i, m in enumerate(models):
                with streams.of(i):
                    _resample_params(m, S[i], param_rngs[i])
            last = it == maxiter - 1
            got, S = draw(it + 1, not last, last)
            if last:
                labels = got
        for m, z in zip(models, labels):
            m.labels_ = z
    finally:
        streams.restore()


class _PythonStreams:
    """_NumpyStreams for Python's global `random` generator (the minibatch indices): model i's stream starts as
    random.seed(python_seeds[i]) and is swapped in (setstate) and out (getstate) around each of its index draws.  Without
    python_seeds the global stream is used as it stands, in model order."""

    def __init__(self, python_seeds, B):
        self.states = None
        if python_seeds is not None:
            python_seeds = _per_model(python_seeds, B, 0, "python seeds")
            self.caller = random.getstate()
            self.states = []
            for sd in python_seeds:
                random.seed(sd)
                self.states.append(random.getstate())
            random.setstate(self.caller)

    @contextmanager
    def of(self, i):
        if self.states is None:
            yield
            return
        random.setstate(self.states[i])
        try:
            yield
        finally:
            self.states[i] = random.getstate()

    def restore(self):
        if self.states is not None:
            random.setstate(self.caller)


def _svi_resident_kind(models, sample_likelihood):
    """What the device-resident SVI loop covers — the families of _resident_reason (mixtures of Gaussians) and of
    _ilr_resident_reason (mixtures of linear-Gaussian experts, one gating kind per batch), without likelihood draws ->
    None for mixtures of Gaussians, else the ILR batch's gating kind.  Raises ValueError naming the model and the reason."""
    if type(models[0]) is BayesianMixtureOfGaussians:
        for i, m in enumerate(models):
            why = _resident_reason(m, sample_likelihood)
            if why is not None:
                raise ValueError(f"resident=True does not cover model {i}: {why}")
        return None
    if sample_likelihood:
        raise ValueError("resident=True does not cover model 0: sample_likelihood=True (the loop makes no per-iteration "
                         "likelihood draws)")
    kinds = []
    for i, m in enumerate(models):
        why, kind = _ilr_resident_reason(m)
        if why is not None:
            raise ValueError(f"resident=True does not cover model {i}: {why}")
        kinds.append(kind)
    if any(k != kinds[0] for k in kinds):
        raise ValueError(f"resident=True takes one gating kind per batch, got {kinds}")
    return kinds[0]


def philox_indices(seed, n_rows, batch_size, t):
    """The minibatch the device draws for one problem at iteration t (index_rng='philox'): slot j holds
    min(int(philox_uniform(seed, j, t) * n_rows), n_rows - 1) — with replacement, any batch_size."""
    from mimo_amd.engine import philox_uniforms
    u = philox_uniforms(seed, np.arange(int(batch_size)), int(t))
    return np.minimum((u * float(n_rows)).astype(np.int64), int(n_rows) - 1)


def _resident_stochastic_descent(models, engine, kind, nrows, first, maxiter, step_size, batch_size, chunk, draw, seeds,
                                 stream):
    """The loop of meanfield_stochastic_descent_batched(resident=True) behind the upload (and the random start, whose
    statistics lie on the device: `first`): priors and the starting posterior up once, svi_run in chunks, state back once.
    draw(): one iteration's B index arrays (index_rng='host'; unused with `seeds`, index_rng='philox'); stream(i): the context
    model i's closing likelihood draws run in."""
    B, K = len(models), models[0].size
    gmm = type(models[0]) is BayesianMixtureOfGaussians
    arr = lambda v: np.asarray(v, dtype=float)
    stack = lambda parts: tuple(np.stack([arr(p[j]) for p in parts]) for j in range(len(parts[0])))
    if gmm:
        engine.vi_set_prior(np.stack([arr(m.gating.prior.alphas) for m in models]),
                            *stack([_native_sweep._prior_block(m.components.prior) for m in models]))
        status = engine.svi_set_state(np.stack([arr(m.gating.posterior.alphas) for m in models]),
                                      *stack([tuple(m.components.posterior.nat_param) for m in models]))
        run, get = engine.svi_run, engine.vi_state
    else:
        stick = kind == 'stick-breaking'
        gate = lambda d: np.stack([arr(getattr(m.gating, d).gammas if stick else getattr(m.gating, d).alphas) for m in models])
        rest = lambda d: np.stack([arr(getattr(m.gating, d).deltas) for m in models]) if stick else None
        engine.vi_ilr_set_prior(kind, gate('prior'), rest('prior'),
                                stack([_native_sweep._prior_block(m.basis.prior) for m in models]),
                                stack([_native_sweep._prior_block(m.models.prior) for m in models]))
        status = engine.svi_ilr_set_state(gate('posterior'), rest('posterior'),
                                          stack([tuple(m.basis.posterior.nat_param) for m in models]),
                                          stack([tuple(m.models.posterior.nat_param) for m in models]))
        run, get = engine.svi_ilr_run, engine.vi_ilr_state

    def check(status):
        for i in np.flatnonzero(status):
            if status[i] & 1:
                raise np.linalg.LinAlgError(f"problem {int(i)}: Matrix is not positive definite (a block of a component's "
                                            "posterior)")
            raise FloatingPointError(f"problem {int(i)}: the canonical form or the bound of its posterior is not finite")

    check(status)
    vlbs = [[] for _ in range(B)]
    scale = np.array([batch_size / float(n) for n in nrows])
    sizes = np.full(B, batch_size, dtype=np.int64)
    left = maxiter
    while left > 0:
        n = min(chunk, left)
        start = first and left == maxiter
        rows = [draw() for _ in range(n - (1 if start else 0))] if seeds is None else None
        trace, n_done, status = run(K, n, step_size, scale, sizes, rows=rows, seeds=seeds, resident_start=start)
        left -= n
        check(status)
        for i in range(B):
            vlbs[i].extend(float(v) for v in trace[:int(n_done[i]), i])
    state = get(K)
    if gmm:
        _write_gmm_state(models, state, vlbs, stream)
    else:
        _write_ilr_state(models, state, vlbs, kind == 'stick-breaking', stream)
    return vlbs


def meanfield_stochastic_descent_batched(models, data, randomize=True, maxiter=500, step_size=1e-3, batch_size=128,
                                         sample_likelihood=True, numpy_seeds=None, python_seeds=None, engine=None,
                                         resident=False, chunk=8, index_rng='host', seeds=None):
    """Stochastic variational inference of B models with two batched passes per outer iteration: per model what its solo
    meanfield_stochastic_descent(data, randomize, maxiter, step_size, batch_size, sample_likelihood=sample_likelihood)
    does in the plain form of the shared outer loop (mixtures/_svi.py).  models / data / engine as in
    meanfield_coordinate_descent_batched; every model's full rows are uploaded once.

    Per iteration: each model draws its minibatch, sample_indices(N_b, batch_size), in model order; ONE pass over the
    chosen rows of all models (engine.estep(..., rows=batches)); each model's natural-gradient step with
    scale = batch_size / N_b; ONE pass over all rows without statistics; each model appends prior terms + bound.  SVI has
    no stopping rule: every model runs maxiter iterations.  Returns the B traces.

    randomize=True: the first step's statistics are those of numpy.random.rand(K, batch_size), normalised over k, on the
    minibatch's rows (the solo start), drawn in model order and passed as a (K, N_b) table that is 0.0 off the minibatch:
    one engine.weighted_stats call that moves K N_b doubles per model to the device, once.

    numpy_seeds[i] / python_seeds[i]: model i's numpy work (the start, the likelihood draws of the steps) and its index
    draws run on streams of their own, started as numpy.random.seed(numpy_seeds[i]) and random.seed(python_seeds[i]), so
    with both lists the batch reproduces B solo runs each preceded by those two calls; the caller's states of both
    generators are restored at the end, also on an exception.  Without a list that generator's global stream is consumed
    in model order (at B = 1: the solo plain form's order).

    resident=True: the natural-gradient step runs on the device too (BatchedHipEngine.svi_run): after the upload (and, with
    randomize=True, the random start exactly as above) the priors and the starting posteriors go up once, the loop runs
    `chunk` iterations per call — minibatch pass, step, pass over all rows, bound, no host work per model — and the
    posteriors come back once and are written into the models as the resident coordinate-descent drivers write them (then
    one _refresh_likelihoods() per model).  Covered: the families of meanfield_coordinate_descent_batched(resident=True) and
    of meanfield_coordinate_descent_batched_ilr, with sample_likelihood=False; anything else raises ValueError naming the
    model and the reason before anything is uploaded or drawn.  index_rng='host': each chunk's indices are drawn with
    sample_indices on the streams above, iteration by iteration and in model order within an iteration, so Python's
    generator is consumed as the host route consumes it (batch_size > N_b raises ValueError).  index_rng='philox': the
    indices are drawn on the device with replacement from the Philox stream keyed by seeds[i] (philox_indices; any
    batch_size), and nothing is sent per chunk.  A problem one of whose blocks is not positive definite raises
    numpy.linalg.LinAlgError naming the problem, one whose canonical form or bound is not finite FloatingPointError."""
    models, data = list(models), list(data)
    kind = _svi_resident_kind(models, sample_likelihood) if resident and models else None      # (sizes aside: the families first)
    models, data, cls = _check_models(models, data)
    B = len(models)
    maxiter, batch_size = int(maxiter), int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size = {batch_size} < 1")
    for name, sd in (("numpy seeds", numpy_seeds), ("python seeds", python_seeds)):
        _per_model(sd, B, 0, name)
    if resident:
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk = {chunk} < 1")
        if index_rng not in ('host', 'philox'):
            raise ValueError(index_rng)
        seeds = [int(sd) for sd in _per_model(seeds, B, 0, "seeds")] if index_rng == 'philox' else None
    rows = [_rows(m, d) for m, d in zip(models, data)]       # (validates the structure before any draw)
    if resident and index_rng == 'host':
        for i, r in enumerate(rows):
            if batch_size > len(r):
                raise ValueError(f"model {i}: batch_size = {batch_size} exceeds its {len(r)} rows (index_rng='host' draws "
                                 "without replacement; index_rng='philox' draws with)")
    nstreams, pstreams = _NumpyStreams(numpy_seeds, B), _PythonStreams(python_seeds, B)
    vlbs = [[] for _ in range(B)]
    if maxiter <= 0:
        return vlbs
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    try:
        engine.upload(rows)
        K = models[0].size
        nrows = [int(n) for n in np.diff(engine.row_off)]
        if resident:
            def draw():
                batches = []
                for i in range(B):
                    with pstreams.of(i):
                        batches.append(sample_indices(nrows[i], batch_size, as_array=True))
                return batches

            first = randomize is True
            if first:       # the random start of the host route below, its statistics left on the device
                batches = draw() if seeds is None else [philox_indices(seeds[i], nrows[i], batch_size, 0) for i in range(B)]
                tables = []
                for i in range(B):
                    with nstreams.of(i):
                        resp = npr.rand(K, len(batches[i]))
                    resp /= np.sum(resp, axis=0)
                    table = np.zeros((K, nrows[i]))
                    np.add.at(table, (slice(None), batches[i]), resp)      # (a row drawn twice counts twice)
                    tables.append(table)
                engine.weighted_stats(tables)
            return _resident_stochastic_descent(models, engine, kind, nrows, first, maxiter, step_size, batch_size, chunk,
                                                draw, seeds, nstreams.of)
        for it in range(maxiter):
            batches = []
            for i in range(B):
                with pstreams.of(i):
                    batches.append(sample_indices(nrows[i], batch_size, as_array=True))
            if it == 0 and randomize is True:
                tables = []
                for i in range(B):
                    with nstreams.of(i):
                        resp = npr.rand(K, len(batches[i]))
                    resp /= np.sum(resp, axis=0)
                    table = np.zeros((K, nrows[i]))
                    table[:, batches[i]] = resp
                    tables.append(table)
                Sb = engine.weighted_stats(tables)
            else:
                Sb, _ = engine.estep(*_stack([m.canonical_expected() for m in models]), rows=batches)
            for i, m in enumerate(models):
                with nstreams.of(i):
                    m._svi_step(Sb[i], batch_size / float(nrows[i]), step_size, sample_likelihood)
            _, sc = engine.estep(*_stack([m.canonical_expected() for m in models]), stats=False)
            for i, m in enumerate(models):
                vlbs[i].append(m._vlb_prior_terms() + sc[i, 0])
        return vlbs
    finally:
        nstreams.restore()
        pstreams.restore()


def meanfield_prediction_batched(models, x, y=None, prediction='average', dist='gaussian', incremental=False,
                                 variance='diagonal', engine=None):
    """meanfield_prediction of B fitted BayesianMixtureOfLinearGaussians in ONE launch (BatchedHipEngine.predict): what the
    reference's parallel job ends with (examples/ilr/evaluate_sinc_parallel.py:196-201: every model's prediction over the
    same inputs).  models: one size and one set of dimensions, affine experts with input_dim, output_dim <= 8 (stacked or
    tied: both expose predictive_blocks()).  x: one (N, dx) array all models predict on (it goes to the device once), or a
    list of B arrays; y (optional: adds nlpd) takes the form of x.  Each model's standardisation is applied in the kernel
    (scale=False: shift 0, scale 1); the host tail is the solo method's (_prediction_tail).  engine: a BatchedHipEngine
    (default: a new one on the device of the first model's engine); nothing it holds is read or changed.
    Returns a list of B tuples, each what the model's solo meanfield_prediction returns — bit for bit."""
    models = list(models)
    B = len(models)
    if B == 0:
        raise ValueError("no models")
    if any(type(m) is not BayesianMixtureOfLinearGaussians for m in models):
        raise ValueError("the models must all be BayesianMixtureOfLinearGaussians")
    models[0]._check_dist(dist)
    if prediction not in ('average', 'mode'):
        raise NotImplementedError(prediction)
    dims = [(m.size, m.input_dim, m.output_dim) for m in models]
    if any(d != dims[0] for d in dims):
        raise ValueError(f"the models differ in size or dimensions: {dims}")
    K, dx, dy = dims[0]
    if any(not m.affine for m in models) or dx > 8 or dy > 8:
        raise NotImplementedError("the batched prediction covers affine experts with input_dim <= 8 and output_dim <= 8 "
                                  f"(got affine = {[bool(m.affine) for m in models]}, input_dim = {dx}, output_dim = {dy})")
    ragged = isinstance(x, (list, tuple))
    if ragged and len(x) != B:
        raise ValueError(f"inputs for {len(x)} models, {B} given")
    if y is not None and isinstance(y, (list, tuple)) != ragged:
        raise ValueError("x and y must take the same form: both one array or both lists of B arrays")
    xs = [np.reshape(xi, (-1, dx)) for xi in x] if ragged else np.reshape(x, (-1, dx))
    ys = None
    if y is not None:
        ys = [np.reshape(yi, (-1, dy)) for yi in y] if ragged else np.reshape(y, (-1, dy))

    def transform(t, scaled, d):
        return np.stack([t.mean_, t.scale_]) if scaled else np.stack([np.zeros(d), np.ones(d)])
    gates = [m._predictive_gate() for m in models]
    blocks = [m.models.predictive_blocks() for m in models]
    stack = lambda parts: np.stack([np.asarray(p, dtype=float) for p in parts])
    c, b, W = (stack([g[i] for g in gates]) for i in range(3))
    Ms, Q, Cc, P, ld = (stack([bl[i] for bl in blocks]) for i in range(5))
    x_tf = np.stack([transform(m.input_transform, m.scale, dx) for m in models])
    y_tf = np.stack([transform(m.output_transform, m.scale, dy) for m in models]) if ys is not None else None
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    diag = variance == 'diagonal'
    res = engine.predict(xs, c, b, W, Ms, Q, Cc, mode=prediction, y=ys, P=P if ys is not None else None,
                         ld=ld if ys is not None else None, variance='diagonal' if diag else 'full',
                         x_transform=x_tf, y_transform=y_tf)
    return [m._prediction_tail(xs[i] if ragged else xs, y, mu, second, nlpd, incremental, diag)
            for i, (m, (mu, second, nlpd)) in enumerate(zip(models, res))]
