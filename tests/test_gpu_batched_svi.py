"""GPU: meanfield_stochastic_descent_batched (mimo_amd/mixtures/batched.py) — B models through one minibatch pass over
chosen rows and one bound pass per outer iteration, against solo meanfield_stochastic_descent runs of the same models after
the same seeds, at the tolerances of the fixtures' own SVI checks (model_checks.check_ilr_svi: 1e-7 on the trace, 1e-6 on
the posterior; check_driver_traces: 1e-8 and 1e-7).  No model's own engine is used during the batched run."""
import os
import random
import subprocess
import sys

import numpy as np
import numpy.random as npr
import pytest

from conftest import ROOT, load_golden, rel_err
from model_checks import build_gmm, build_ilr
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine
from mimo_amd.mixtures.batched import meanfield_stochastic_descent_batched

pytestmark = pytest.mark.gpu

ITERS = 12
# (fixture, step size of the fixture's SVI run, trace tolerance, posterior tolerance)
CASES = [("ilr_svi_dx2_dy1_k8", 5e-1, 1e-7, 1e-6), ("drivers_d3_k5_dir", 5e-2, 1e-8, 1e-7)]
NUMPY_SEEDS, PYTHON_SEEDS = [5, 5, 6, 7], [15, 15, 16, 17]


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


def _models(name, engine, B=4):
    """B models of the fixture: copies 0 .. 1 on the fixture's data, the rest on perturbed data.  ILR: the scaling transform
    and the seeded Gibbs warm-up of the fixture's own flow, per model."""
    g = load_golden(name)
    rng = np.random.default_rng(3)
    models, data = [], []
    for i in range(B):
        if name.startswith("drivers"):
            m = build_gmm(g, engine)[1]
            d = g["X"] if i < 2 else g["X"] + 0.05 * (i - 1) * rng.standard_normal(g["X"].shape)
        else:
            m = build_ilr(g, engine)[1]
            X, Y = g["X"], g["Y"]
            if i >= 2:
                X = X + 0.05 * (i - 1) * rng.standard_normal(X.shape)
                Y = Y + 0.05 * (i - 1) * rng.standard_normal(Y.shape)
            m.init_transform(X, Y)
            npr.seed(int(g["seed"]) + 1)
            m.resample(X, Y, init_labels='random', maxiter=3, progress_bar=False)
            d = (X, Y)
        models.append(m)
        data.append(d)
    return models, data


def _posterior(m):
    post = m.components.posterior if hasattr(m, "components") else m.models.posterior
    return post.params


def _refuse(*a, **kw):
    raise AssertionError("a model's own engine was used during the batched run")


@pytest.mark.parametrize("randomize", [False, True])
@pytest.mark.parametrize("name,step,tol,ptol", CASES)
def test_batched_svi_equals_solo_runs(engine, beng, monkeypatch, name, step, tol, ptol, randomize):
    kw = dict(randomize=randomize, maxiter=ITERS, step_size=step, batch_size=64)
    models, data = _models(name, engine)
    with monkeypatch.context() as mp:
        for what in ("upload", "estep", "weighted_stats"):
            mp.setattr(HipEngine, what, _refuse)
        vlbs = meanfield_stochastic_descent_batched(models, data, numpy_seeds=NUMPY_SEEDS, python_seeds=PYTHON_SEEDS,
                                                    engine=beng, **kw)
    assert [len(v) for v in vlbs] == [ITERS] * len(models)
    assert vlbs[0] == vlbs[1]                                   # identical copies, identical seeds: bit-identical traces
    assert all(np.array_equal(a, b) for a, b in zip(_posterior(models[0]), _posterior(models[1])))
    solos, _ = _models(name, engine)
    worst = [0., 0.]
    for m, s, d, ns, ps, v in zip(models, solos, data, NUMPY_SEEDS, PYTHON_SEEDS, vlbs):
        npr.seed(ns)
        random.seed(ps)
        vs = s.meanfield_stochastic_descent(*(d if isinstance(d, tuple) else (d,)), progress_bar=False, **kw)
        worst[0] = max(worst[0], rel_err(np.array(v), np.array(vs)))
        worst[1] = max([worst[1]] + [rel_err(a, b) for a, b in zip(_posterior(m), _posterior(s))])
    print(f"{name} randomize={randomize}: largest difference to the solo runs: trace {worst[0]:.2e}, posterior {worst[1]:.2e}")
    assert worst[0] < tol and worst[1] < ptol


def test_example_runs_the_stochastic_flow():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ilr_sinc_batched.py"), "--fits", "3", "--rows", "400",
                          "--experts", "8", "--svi-iters", "5"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "3 fits of 320 rows, K = 8" in out.stdout and "iterations 5 - 5" in out.stdout
