"""Mean-field coordinate descent and Gibbs sampling of B independent mixtures with ONE batched pass per iteration / sweep
(mimo_amd.batched.BatchedHipEngine): what the reference does with joblib.Parallel over B fits
(examples/ilr/evaluate_sinc_parallel.py) or with random restarts of one model.

VI: per iteration each model runs the host step of its own meanfield_iteration, in model order (conjugate update — the
native sweep where it applies —, canonical form), then one batched pass over all B data sets, then, per model, the
likelihood draws, the prior terms of the bound and the bound itself.  A model stops at the iteration where its solo
run would stop; after that it is neither updated nor appended to (its last parameters stay in the batch).

Gibbs: per sweep each model runs the host half of its solo resample sweep, in model order (parameter and gating draws,
canonical form, host uniforms), then one batched label pass draws every model's labels and their statistics."""
from contextlib import contextmanager

import numpy as np
import numpy.random as npr

from mimo_amd.batched import BatchedHipEngine
from mimo_amd.distributions import native_sweep as _native_sweep
from mimo_amd.distributions.lingauss import joint_rows
from mimo_amd.mixtures.gmm import BayesianMixtureOfGaussians, _component_stats
from mimo_amd.mixtures.ilr import BayesianMixtureOfLinearGaussians


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


def meanfield_coordinate_descent_batched(models, data, randomize=True, maxiter=250, tol=1e-8, init_rng='host', seeds=None,
                                         sample_likelihood=True, engine=None):
    """models: B BayesianMixtureOfGaussians with data a list of B `obs`, or B BayesianMixtureOfLinearGaussians with data a
    list of B `(x, y)`; one class, one size and one set of dimensions for all.  randomize / init_rng / seeds[i] /
    sample_likelihood as in the solo drivers (the random start is one batched table pass: the host draws are made in
    model order).  engine: a
    BatchedHipEngine (default: a new one on the device of the first model's engine).  Returns the B ELBO traces."""
    models, data, cls = _check_models(models, data)
    B = len(models)
    seeds = _per_model(seeds, B, 0, "seeds")
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    engine.upload([_rows(m, d) for m, d in zip(models, data)])

    if randomize:
        S = _random_start(engine, models[0].size, init_rng, seeds)
    else:
        canons = [m.canonical_expected() for m in models]
        S, _ = engine.estep(*_stack(canons))
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
