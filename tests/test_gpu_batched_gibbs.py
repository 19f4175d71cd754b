"""GPU: the batched Gibbs label pass (mimo_gibbs_labels_batched / mimo_label_stats_batched, BatchedHipEngine.gibbs_labels /
label_stats) against the oracle and B solo label passes; independence and determinism; loud failures; the resample_batched
driver against the reference fixtures and against solo runs; the example's Gibbs warm-up."""
import os
import random
import subprocess
import sys

import numpy as np
import numpy.random as npr
import pytest

from batched_checks import TOL, check_stats, qerr
from batched_checks import problems as random_problems
from conftest import ROOT, load_golden, rel_err
import model_checks as mc
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine, _ptr
from mimo_amd.mixtures.batched import resample_batched
from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def solo():
    return HipEngine(0)


def problems(rng, rows, D, K):
    """The shared random batch with component 1 of every problem switched off (c = -inf)."""
    return random_problems(rng, rows, D, K, off=1)


ROWS = [0, 1, 31, 33, 2500]
CELLS = [(1, 6), (2, 100), (3, 17), (8, 64), (11, 128), (12, 64), (16, 64)]


@pytest.mark.parametrize("D,K", CELLS)
def test_labels_and_stats_against_oracle_and_solo(beng, solo, D, K):
    rng = np.random.default_rng(100 * D + K)
    rows = [int(n) for n in rng.permutation(ROWS)]
    Zs, c, b, W = problems(rng, rows, D, K)
    beng.upload(Zs)
    seeds = [int(s) for s in rng.integers(0, 2**63, size=len(rows))]
    u = [rng.random((1, n)) for n in rows]
    for mode in ("host", "philox"):
        labs, S = beng.gibbs_labels(c, b, W, seeds=seeds if mode == "philox" else None, sweep=5,
                                    u=u if mode == "host" else None)
        for i, n in enumerate(rows):
            Z = Zs[i]
            uu = u[i].reshape(-1) if mode == "host" else O.philox_uniforms(seeds[i], np.arange(n), 5)
            ref = O.sample_discrete_from_log(O.canonical_eval(Z, c[i], b[i], W[i]), uu) if n else np.zeros(0, np.int32)
            assert labs[i].dtype == np.int32 and np.array_equal(labs[i], ref), (mode, i, n)
            if K > 2:
                assert not np.any(labs[i] == 1)            # c = -inf: never drawn
            check_stats(S[i], Z, labs[i], K)
            if n:
                solo.upload(Z)
                sl, sS = solo.gibbs_labels(c[i], b[i], W[i], seed=seeds[i], sweep=5,
                                           u=u[i] if mode == "host" else None)
                assert np.array_equal(sl, labs[i])
                assert np.array_equal(sS.n, S[i].n)
                assert qerr(S[i].sx, sS.sx) <= TOL and qerr(S[i].sxx, sS.sxx) <= TOL
        # the labels stay resident: mimo_get_labels returns the concatenation, label_stats(None) their statistics
        assert np.array_equal(np.concatenate(beng.get_labels()), np.concatenate(labs))
        S2 = beng.label_stats(None, K)
        for i in range(len(rows)):
            assert np.array_equal(S2[i].packed(), S[i].packed())
    # labels only
    labs2, none = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=5, stats=False)
    assert none is None and all(np.array_equal(x, y) for x, y in zip(labs2, labs))


@pytest.mark.parametrize("D,K", [(2, 100), (12, 64)])
def test_independence_and_determinism(beng, D, K):
    rng = np.random.default_rng(7 + D)
    rows = [2500, 33, 0, 31, 1]
    Zs, c, b, W = problems(rng, rows, D, K)
    seeds = [11, 12, 13, 14, 15]
    u = [rng.random(n) for n in rows]
    beng.upload(Zs)
    Lb, Sb = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=3)
    Lb2, Sb2 = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=3)
    Hb, HSb = beng.gibbs_labels(c, b, W, u=u)
    for i in range(5):
        assert np.array_equal(Lb[i], Lb2[i]) and np.array_equal(Sb[i].packed(), Sb2[i].packed())
    for i in (0, 1, 3):
        beng.upload([Zs[i]])
        La, Sa = beng.gibbs_labels(c[i:i + 1], b[i:i + 1], W[i:i + 1], seeds=[seeds[i]], sweep=3)
        Ha, HSa = beng.gibbs_labels(c[i:i + 1], b[i:i + 1], W[i:i + 1], u=[u[i]])
        assert np.array_equal(La[0], Lb[i]) and np.array_equal(Sa[0].packed(), Sb[i].packed())
        assert np.array_equal(Ha[0], Hb[i]) and np.array_equal(HSa[0].packed(), HSb[i].packed())


def test_given_labels(beng):
    rng = np.random.default_rng(21)
    D, K = 3, 17
    rows = [33, 0, 2500, 1]
    Zs, c, b, W = problems(rng, rows, D, K)
    beng.upload(Zs)
    for kind in ("one", "three", "random"):
        if kind == "one":
            labels = [np.full(n, 5, dtype=np.int32) for n in rows]
        elif kind == "three":
            labels = [rng.choice([0, 7, 16], size=n).astype(np.int32) for n in rows]
        else:
            labels = [rng.integers(0, K, size=n) for n in rows]
        S = beng.label_stats(labels, K)
        for i, n in enumerate(rows):
            check_stats(S[i], Zs[i], labels[i], K)


def test_loud_failures(beng, solo):
    rng = np.random.default_rng(31)
    for D, K in ((16, 65), (2, 129)):
        Zs, c, b, W = problems(rng, [40, 3], D, K)
        beng.upload(Zs)
        with pytest.raises(_lib.MimoHipError):
            beng.gibbs_labels(c, b, W, seeds=[1, 2])
        with pytest.raises(_lib.MimoHipError):
            beng.label_stats([np.zeros(40, np.int32), np.zeros(3, np.int32)], K)
    Zs, c, b, W = problems(rng, [40, 3], 3, 4)
    beng.upload(Zs)
    beng.set_structure('diag')
    try:
        with pytest.raises(_lib.MimoHipError):
            beng.gibbs_labels(c, b, W * np.eye(3), seeds=[1, 2])
        with pytest.raises(_lib.MimoHipError):
            beng.label_stats([np.zeros(40, np.int32), np.zeros(3, np.int32)], 4)
    finally:
        beng.set_structure('full')
    lib, ctx = beng._lib, beng._ctx
    S = np.empty((2, 4, 13)); lab = np.empty(43, dtype=np.int32)
    # seeds and u both NULL
    assert lib.mimo_gibbs_labels_batched(ctx, _ptr(c), _ptr(b), _ptr(W), 4, None, 0, None, 0, _ptr(lab), _ptr(S)) == _lib.E_INVALID
    # labels out of range (the library checks too)
    bad = np.zeros(43, dtype=np.int32); bad[41] = 4
    assert lib.mimo_label_stats_batched(ctx, _ptr(bad), 4, 0, _ptr(S)) == _lib.E_INVALID
    for name, val in (("c", np.nan), ("c", np.inf), ("W", np.nan)):
        p = {"c": c.copy(), "b": b.copy(), "W": W.copy()}
        p[name].flat[2] = val
        with pytest.raises(_lib.MimoHipError):
            beng.gibbs_labels(p["c"], p["b"], p["W"], seeds=[1, 2])
    # engine-side validation: seed count, uniform lengths, label lengths and ranges
    for kw in ({"seeds": [1]}, {}, {"u": [np.zeros(40)]}, {"u": [np.zeros(40), np.zeros(4)]}):
        with pytest.raises(ValueError):
            beng.gibbs_labels(c, b, W, **kw)
    for labels in ([np.zeros(40, np.int32)], [np.zeros(40, np.int32), np.zeros(2, np.int32)],
                   [np.zeros(40, np.int32), np.array([0, 4, 1])], [np.zeros(40, np.int32), np.array([0, -1, 1])]):
        with pytest.raises(ValueError):
            beng.label_stats(labels, 4)
    # the single-problem context refuses the batched calls
    solo.upload(np.ascontiguousarray(Zs[0]))
    sd = np.array([1, 2], dtype=np.uint64)
    assert lib.mimo_gibbs_labels_batched(solo._ctx, _ptr(c), _ptr(b), _ptr(W), 4, _ptr(sd), 0, None, 0, _ptr(lab),
                                         _ptr(S)) == _lib.E_INVALID
    assert lib.mimo_label_stats_batched(solo._ctx, _ptr(lab), 4, 0, _ptr(S)) == _lib.E_INVALID
    # and the batch still runs after all of that
    labs, S = beng.gibbs_labels(c, b, W, seeds=[1, 2])
    assert [len(z) for z in labs] == [40, 3]


# ---- driver --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["gibbs_c1_trace", "gibbs_stick_trace"])
def test_driver_reproduces_gibbs_trace(solo, name):
    solo.set_structure('full')
    g = load_golden(name)
    X = g["X"]
    kind, model = mc.build_gmm(g, solo)
    model.components.likelihood.params = (g["lik0_mus"], g["lik0_lmbdas"])
    model.gating.likelihood.params = g["lik0_probs"].copy()
    npr.seed(int(g["seed2"]))
    resample_batched([model], [X], init_labels='prior', maxiter=5, label_rng='host')
    assert np.array_equal(model.labels_, g["s4_labels"])
    assert rel_err(model.components.likelihood.mus, g["driver_mus"]) < 1e-8
    assert rel_err(model.gating.likelihood.probs, g["driver_probs"]) < 1e-10


def test_driver_reproduces_ilr_gibbs_prefix(solo):
    solo.set_structure('full')
    g = load_golden("ilr_svi_dx2_dy1_k8")
    kind, ilr = mc.build_ilr(g, solo)
    ilr.init_transform(g["X"], g["Y"])
    npr.seed(int(g["seed"]) + 1)
    random.seed(int(g["seed"]) + 2)
    resample_batched([ilr], [(g["X"], g["Y"])], init_labels='random', maxiter=3)
    assert rel_err(ilr.gating.likelihood.probs, g["gibbs_probs"]) < 1e-9
    assert rel_err(ilr.models.likelihood.As, g["gibbs_As"]) < 1e-7


@pytest.mark.parametrize("label_rng", ["host", "philox"])
def test_driver_against_solo_runs(solo, label_rng):
    solo.set_structure('full')
    g = load_golden("gibbs_stick_trace")
    X = g["X"]
    sizes = [400, 250, 400, 97, 400]                 # models 0 and 2: identical copies
    numpy_seeds = [5, 6, 5, 7, 8]
    seeds = [3, 4, 3, 9, 10]

    def fresh():
        kind, m = mc.build_gmm(g, solo)
        m.components.likelihood.params = (g["lik0_mus"], g["lik0_lmbdas"])
        m.gating.likelihood.params = g["lik0_probs"].copy()
        return m

    ref = []
    for n, ns, sd in zip(sizes, numpy_seeds, seeds):
        m = fresh()
        npr.seed(ns)
        m.resample(X[:n], init_labels='prior', maxiter=3, progress_bar=False, label_rng=label_rng, seed=sd)
        ref.append(m)
    models = [fresh() for _ in sizes]
    npr.seed(1234)
    npr.normal()                                     # (a cached gaussian in the caller's state)
    before = npr.get_state()
    resample_batched(models, [X[:n] for n in sizes], init_labels='prior', maxiter=3, label_rng=label_rng, seeds=seeds,
                     numpy_seeds=numpy_seeds)
    after = npr.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    for m, r in zip(models, ref):
        assert np.array_equal(m.labels_, r.labels_)
        assert rel_err(m.components.likelihood.mus, r.components.likelihood.mus) < 1e-8
        assert rel_err(m.components.likelihood.lmbdas, r.components.likelihood.lmbdas) < 1e-8
        assert rel_err(m.gating.likelihood.probs, r.gating.likelihood.probs) < 1e-8
    assert np.array_equal(models[0].labels_, models[2].labels_)
    assert np.array_equal(models[0].components.likelihood.mus, models[2].components.likelihood.mus)
    assert np.array_equal(models[0].components.likelihood.lmbdas, models[2].components.likelihood.lmbdas)


def test_example_gibbs_warmup_runs():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ilr_sinc_batched.py"), "--rows", "300", "--fits", "4",
           "--experts", "16", "--iters", "5", "--gibbs-iters", "3"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert "Gibbs warm-up" in proc.stdout
