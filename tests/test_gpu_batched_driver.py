"""GPU: meanfield_coordinate_descent_batched (mimo_amd/mixtures/batched.py) — B models through one batched pass per
iteration against the reference's VI traces and against solo meanfield_coordinate_descent runs of the same models."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from model_checks import build_gmm, load_gmm_state, build_ilr, load_ilr_state
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched

pytestmark = pytest.mark.gpu

# (fixture, trace tolerance of check_gmm_vi_trace / check_ilr_vi_trace)
CASES = [("gmm_c1_d2_k4_dir", 1e-8), ("gmm_c3_d8_k32_stick", 1e-8), ("ilr_dx1_dy1_k6_dir", 1e-7),
         ("ilr_dx1_dy1_k50_stick", 1e-7)]


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


def _models(name, engine, B=4):
    """B copies of the fixture's model at its loaded state: copies 0 .. 1 on the fixture's data, the rest on perturbed data."""
    g = load_golden(name)
    rng = np.random.default_rng(3)
    models, data = [], []
    for i in range(B):
        if name.startswith("gmm"):
            kind, m = build_gmm(g, engine)
            load_gmm_state(m, g, kind)
            X = g["X"] if i < 2 else g["X"] + 0.05 * (i - 1) * rng.standard_normal(g["X"].shape)
            data.append(X)
        else:
            kind, m = build_ilr(g, engine)
            load_ilr_state(m, g, kind)
            X, Y = g["X"], g["Y"]
            if i >= 2:
                X = X + 0.05 * (i - 1) * rng.standard_normal(X.shape)
                Y = Y + 0.05 * (i - 1) * rng.standard_normal(Y.shape)
            data.append((X, Y))
        models.append(m)
    return g, models, data


def _solo(m, d, **kw):
    if isinstance(d, tuple):
        return m.meanfield_coordinate_descent(d[0], d[1], progress_bar=False, **kw)
    return m.meanfield_coordinate_descent(d, progress_bar=False, **kw)


def _posterior(m):
    post = m.components.posterior if hasattr(m, "components") else m.models.posterior
    return post.params


@pytest.mark.parametrize("name,tol", CASES)
def test_batched_driver_reproduces_fixture_and_solo_runs(engine, beng, name, tol):
    g, models, data = _models(name, engine)
    n = len(g["vi_vlb"])
    vlbs = meanfield_coordinate_descent_batched(models, data, randomize=False, tol=0., maxiter=n, engine=beng)
    assert [len(v) for v in vlbs] == [n] * len(models)
    for v in vlbs[:2]:
        assert rel_err(np.array(v), g["vi_vlb"]) < tol
    assert vlbs[0] == vlbs[1]                                   # identical copies: bit-identical traces
    # every model's trace and final posterior equal a solo run of the same model from the same state
    _, solos, _ = _models(name, engine)
    for m, s, d, v in zip(models, solos, data, vlbs):
        vs = _solo(s, d, randomize=False, tol=0., maxiter=n)
        assert rel_err(np.array(v), np.array(vs)) < 1e-10
        for a, b in zip(_posterior(m), _posterior(s)):
            assert rel_err(a, b) < 1e-8


@pytest.mark.parametrize("name", ["gmm_c1_d2_k4_dir", "ilr_dx1_dy1_k6_dir"])
def test_batched_driver_philox_starts_and_stopping(engine, beng, name):
    _, models, data = _models(name, engine, B=5)
    seeds = [11, 11, 12, 13, 14]
    kw = dict(randomize=True, init_rng="philox", tol=1e-2, maxiter=60)
    vlbs = meanfield_coordinate_descent_batched(models, data, seeds=seeds, engine=beng, **kw)
    _, solos, _ = _models(name, engine, B=5)
    lengths = []
    for m, s, d, seed, v in zip(models, solos, data, seeds, vlbs):
        vs = _solo(s, d, seed=seed, **kw)
        assert len(v) == len(vs)
        assert rel_err(np.array(v), np.array(vs)) < 1e-10
        for a, b in zip(_posterior(m), _posterior(s)):
            assert rel_err(a, b) < 1e-8
        lengths.append(len(v))
    assert vlbs[0] == vlbs[1]
    assert len(set(lengths)) > 1, f"all models stopped after {lengths[0]} iterations: the run does not test the stopping rule"
