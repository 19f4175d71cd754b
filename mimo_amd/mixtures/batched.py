"""Mean-field coordinate descent of B independent mixtures with ONE batched softmax pass per iteration
(mimo_amd.batched.BatchedHipEngine): what the reference does with joblib.Parallel over B fits
(examples/ilr/evaluate_sinc_parallel.py) or with random restarts of one model.

Per iteration each model runs the host step of its own meanfield_iteration, in model order (conjugate update — the
native sweep where it applies —, canonical form), then one batched pass over all B data sets, then, per model, the
likelihood draws, the prior terms of the bound and the bound itself.  A model stops at the iteration where its solo
run would stop; after that it is neither updated nor appended to (its last parameters stay in the batch)."""
import numpy as np

from mimo_amd.batched import BatchedHipEngine
from mimo_amd.distributions import native_sweep as _native_sweep
from mimo_amd.distributions.lingauss import joint_rows
from mimo_amd.mixtures.gmm import BayesianMixtureOfGaussians, _component_stats, random_start
from mimo_amd.mixtures.ilr import BayesianMixtureOfLinearGaussians


def _rows(model, d):
    """The model's data rows as its solo driver uploads them (ILR: scaled per model, z = [x, y])."""
    if isinstance(model, BayesianMixtureOfGaussians):
        if model._structure() != 'full':
            raise ValueError("the batched pass covers symmetric precision blocks only (full structure)")
        return np.ascontiguousarray(np.asarray(d, dtype=float).reshape(-1, model.dim))
    x, y = d
    return np.ascontiguousarray(joint_rows(*model._scaled(x, y)))


def _bind(model, d):
    if isinstance(model, BayesianMixtureOfGaussians):
        return model._bind(d)
    return model._bind(*model._scaled(*d))


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


def meanfield_coordinate_descent_batched(models, data, randomize=True, maxiter=250, tol=1e-8, init_rng='host', seeds=None,
                                         sample_likelihood=True, engine=None):
    """models: B BayesianMixtureOfGaussians with data a list of B `obs`, or B BayesianMixtureOfLinearGaussians with data a
    list of B `(x, y)`; one class, one size and one set of dimensions for all.  randomize / init_rng / seeds[i] /
    sample_likelihood as in the solo drivers (the random start runs on each model's own engine).  engine: a
    BatchedHipEngine (default: a new one on the device of the first model's engine).  Returns the B ELBO traces."""
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
    seeds = [0] * B if seeds is None else list(seeds)
    if len(seeds) != B:
        raise ValueError(f"{len(seeds)} seeds for {B} models")
    if engine is None:
        engine = BatchedHipEngine(getattr(models[0].engine, 'device', 0))
    engine.upload([_rows(m, d) for m, d in zip(models, data)])

    if randomize:
        S = [random_start(_bind(m, d), m.size, init_rng, s) for m, d, s in zip(models, data, seeds)]
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
